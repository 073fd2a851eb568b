// A stand-alone program around the host JPEG decoder (fastvim_amd/csrc/jpeg_host.cpp), meant to be built together with it
// by the host compiler with -fsanitize=address,undefined and run on the CPU (tests/test_jpeg_host_sanitize_cpu.py):
//
//   jpeg_host_check FILE...
//
// Every FILE goes through fv_jpeg_probe and, if served, through fv_jpeg_entropy_decode for the whole image, for an inner
// window, and with one element of capacity too few (which must be refused).  Then every truncation of the first FILE, and
// 4000 seeded byte mutations of the FILEs in turn.  Inputs and outputs live in heap blocks of exactly the size passed, so
// a read or write one byte outside is a sanitizer report.  Exit status 0: all FILEs behaved and nothing was reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/fastvim_hip.h"

namespace {

constexpr long long kMaxElems = 1ll << 22;      // a mutated header may claim 65535 x 65535

long long elements(const int* info, const int* win) {
  const int cls = info[3];
  const long long per = cls == FV_JPEG_GRAY ? 1 : cls == FV_JPEG_444 ? 3 : cls == FV_JPEG_422 ? 4 : 6;
  return (long long)win[2] * win[3] * per * 64;
}

// probe + decode of an exact-size copy; returns the decoder's code (or 1 for an unserved file)
int decode(const uint8_t* src, long long n, bool inner, long long short_by, long long* checksum) {
  uint8_t* data = (uint8_t*)malloc(n ? (size_t)n : 1);
  memcpy(data, src, (size_t)n);
  int info[FV_JPEG_INFO_INTS];
  int rc = fv_jpeg_probe(data, n, info);
  if (rc == FV_OK && !info[4]) rc = 1;
  if (rc == FV_OK) {
    int win[4] = {0, 0, info[6], info[7]};
    if (inner && info[6] > 2 && info[7] > 2) { win[0] = 1; win[1] = 1; win[2] = info[6] - 2; win[3] = info[7] - 2; }
    long long cap = elements(info, win) - short_by;
    if (cap > kMaxElems) cap = kMaxElems;
    if (cap < 0) cap = 0;
    int16_t* coef = (int16_t*)malloc(cap ? (size_t)cap * 2 : 1);
    int record[FV_JPEG_REC_INTS];
    rc = fv_jpeg_entropy_decode(data, n, win, coef, cap, record);
    if (rc == FV_OK && checksum)
      for (long long k = 0; k < cap; ++k) *checksum += coef[k];
    free(coef);
  }
  free(data);
  return rc;
}

}  // namespace

int main(int argc, char** argv) {
  std::vector<std::vector<uint8_t>> files;
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
    std::vector<uint8_t> d;
    uint8_t buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) d.insert(d.end(), buf, buf + got);
    fclose(f);
    files.push_back(d);
  }
  if (files.empty()) { fprintf(stderr, "usage: jpeg_host_check FILE...\n"); return 2; }
  long long sum = 0;
  int served = 0, bad = 0;
  for (size_t k = 0; k < files.size(); ++k) {
    const std::vector<uint8_t>& d = files[k];
    const int rc = decode(d.data(), (long long)d.size(), false, 0, &sum);
    if (rc == 1) continue;                                       // unserved: the probe's answer, not a failure
    ++served;
    if (rc != FV_OK) { fprintf(stderr, "%s: whole image: code %d\n", argv[k + 1], rc); ++bad; }
    if (decode(d.data(), (long long)d.size(), true, 0, &sum) != FV_OK) { fprintf(stderr, "%s: inner window failed\n", argv[k + 1]); ++bad; }
    if (decode(d.data(), (long long)d.size(), false, 1, &sum) != FV_JPEG_E_CAPACITY) { fprintf(stderr, "%s: short capacity accepted\n", argv[k + 1]); ++bad; }
  }
  int trunc_ok = 0;
  for (size_t n = 0; n < files[0].size(); ++n)
    if (decode(files[0].data(), (long long)n, false, 0, &sum) == FV_OK) ++trunc_ok;
  uint64_t state = 0x9E3779B97F4A7C15ull;
  auto next = [&state]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(state >> 33); };
  int mut_ok = 0;
  for (int it = 0; it < 4000; ++it) {
    std::vector<uint8_t> d = files[it % files.size()];
    const int edits = 1 + next() % 3;
    for (int e = 0; e < edits; ++e) d[next() % d.size()] = (uint8_t)next();
    if (decode(d.data(), (long long)d.size(), (it & 1) != 0, 0, &sum) == FV_OK) ++mut_ok;
  }
  printf("files %zu served %d bad %d; truncations decoded %d of %zu; mutations decoded %d of 4000; checksum %lld\n",
         files.size(), served, bad, trunc_ok, files[0].size(), mut_ok, sum);
  return bad ? 1 : 0;
}
