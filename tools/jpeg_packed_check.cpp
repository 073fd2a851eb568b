// A stand-alone program around the PACKED entry point of the host JPEG decoder (fastvim_amd/csrc/jpeg_host.cpp,
// fv_jpeg_entropy_decode_packed), meant to be built together with it by the host compiler with
// -fsanitize=address,undefined and run on the CPU (tests/test_jpeg_packed_sanitize_cpu.py):
//
//   jpeg_packed_check FILE...
//
// Every FILE goes through fv_jpeg_probe and, if served, through the packed decoder for the whole image and for an inner
// window.  Then every truncation of the first FILE, and 4000 seeded byte mutations of the FILEs in turn.  Each of these
// runs TWICE: with an output buffer of exactly fv_jpeg_packed_bound(blocks) bytes, and with one of a third of that.
// Inputs and outputs live in heap blocks of exactly the size passed, so a read or write one byte outside is a sanitizer
// report.  A successful result is walked the way the format is specified (headers, offsets, values inside the bytes
// written), and the third-of-the-bound run must agree with the exact-bound run: the same bytes, or FV_JPEG_E_CAPACITY
// exactly when the result does not fit.  Exit status 0: all FILEs behaved and nothing was reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/fastvim_hip.h"

namespace {

constexpr long long kMaxBytes = 1ll << 24;      // a mutated header may claim 65535 x 65535

long long blocks_of(const int* info, const int* win) {
  const int cls = info[3];
  const long long per = cls == FV_JPEG_GRAY ? 1 : cls == FV_JPEG_444 ? 3 : cls == FV_JPEG_422 ? 4 : 6;
  return (long long)win[2] * win[3] * per;
}

long long i64(const int* r, int at) { return (long long)(((uint64_t)(uint32_t)r[at + 1] << 32) | (uint32_t)r[at]); }

// the result as the format states it: false where a header or a value lies outside the bytes written
bool well_formed(const uint8_t* out, const int* rec, long long* checksum) {
  const long long blocks = rec[17], end = i64(rec, 15), hb = i64(rec, 25), vb = i64(rec, 27);
  if (rec[0] != 2 || hb != 0 || vb != 16 * blocks || end < vb || (end & 1)) return false;
  long long cur = vb;
  for (long long b = 0; b < blocks; ++b) {
    uint32_t w[4];
    memcpy(w, out + 16 * b, 16);
    const uint64_t mask = (uint64_t)w[1] << 32 | w[0];
    const int wide = (int)(w[2] >> 31), n = __builtin_popcountll(mask);
    const long long off = vb + (w[2] & 0x7fffffffu), bytes = (long long)n << wide;
    if ((mask & 1) || (w[3] >> 16) || off != cur || off + bytes + (bytes & 1) > end) return false;
    bool any_wide = false;
    for (int k = 0; k < n; ++k) {
      int v;
      if (wide) { int16_t t; memcpy(&t, out + off + 2 * k, 2); v = t; } else { v = (int8_t)out[off + k]; }
      if (v == 0) return false;
      any_wide = any_wide || v < -128 || v > 127;
      *checksum += v;
    }
    if (any_wide != (wide != 0) || ((bytes & 1) && out[off + bytes] != 0)) return false;
    cur = off + bytes + (bytes & 1);
  }
  return cur == end;
}

// probe + packed decode of an exact-size copy, into an exact-bound buffer and into a third of it; returns the code of
// the exact-bound run (1: unserved), -100 where a result is malformed or the two runs disagree
int decode(const uint8_t* src, long long n, bool inner, long long* checksum) {
  uint8_t* data = (uint8_t*)malloc(n ? (size_t)n : 1);
  memcpy(data, src, (size_t)n);
  int info[FV_JPEG_INFO_INTS];
  int rc = fv_jpeg_probe(data, n, info);
  if (rc == FV_OK && !info[4]) rc = 1;
  if (rc == FV_OK) {
    int win[4] = {0, 0, info[6], info[7]};
    if (inner && info[6] > 2 && info[7] > 2) { win[0] = 1; win[1] = 1; win[2] = info[6] - 2; win[3] = info[7] - 2; }
    long long bound = fv_jpeg_packed_bound(blocks_of(info, win));
    if (bound > kMaxBytes) bound = kMaxBytes;
    const long long third = bound / 3;
    // posix_memalign: 16-byte aligned as the entry point asks, and of exactly the size passed
    void *full_v = nullptr, *small_v = nullptr;
    if (posix_memalign(&full_v, 16, bound ? (size_t)bound : 1) != 0 || posix_memalign(&small_v, 16, third ? (size_t)third : 1) != 0) {
      fprintf(stderr, "out of memory\n");
      exit(2);
    }
    uint8_t *full = (uint8_t*)full_v, *small = (uint8_t*)small_v;
    int record[FV_JPEG_REC_INTS], record3[FV_JPEG_REC_INTS];
    rc = fv_jpeg_entropy_decode_packed(data, n, win, full, bound, record);
    const int rc3 = fv_jpeg_entropy_decode_packed(data, n, win, small, third, record3);
    if (rc == FV_OK) {
      const long long end = i64(record, 15);
      if (!well_formed(full, record, checksum)) rc = -100;
      else if (end <= third ? (rc3 != FV_OK || memcmp(record, record3, sizeof(record)) != 0 || memcmp(full, small, (size_t)end) != 0)
                            : rc3 != FV_JPEG_E_CAPACITY) rc = -100;
    } else if (rc3 != rc && rc3 != FV_JPEG_E_CAPACITY) {
      rc = -100;                                 // an error of the file is the same error, unless the headers already do not fit
    }
    free(full);
    free(small);
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
  if (files.empty()) { fprintf(stderr, "usage: jpeg_packed_check FILE...\n"); return 2; }
  long long sum = 0;
  int served = 0, bad = 0;
  for (size_t k = 0; k < files.size(); ++k) {
    const std::vector<uint8_t>& d = files[k];
    const int rc = decode(d.data(), (long long)d.size(), false, &sum);
    if (rc == 1) continue;                                       // unserved: the probe's answer, not a failure
    ++served;
    if (rc != FV_OK) { fprintf(stderr, "%s: whole image: code %d\n", argv[k + 1], rc); ++bad; }
    if (decode(d.data(), (long long)d.size(), true, &sum) != FV_OK) { fprintf(stderr, "%s: inner window failed\n", argv[k + 1]); ++bad; }
  }
  int trunc_ok = 0;
  for (size_t n = 0; n < files[0].size(); ++n) {
    const int rc = decode(files[0].data(), (long long)n, false, &sum);
    if (rc == FV_OK) ++trunc_ok;
    if (rc == -100) { fprintf(stderr, "truncation at %zu: malformed result\n", n); ++bad; }
  }
  uint64_t state = 0x9E3779B97F4A7C15ull;
  auto next = [&state]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(state >> 33); };
  int mut_ok = 0;
  for (int it = 0; it < 4000; ++it) {
    std::vector<uint8_t> d = files[it % files.size()];
    const int edits = 1 + next() % 3;
    for (int e = 0; e < edits; ++e) d[next() % d.size()] = (uint8_t)next();
    const int rc = decode(d.data(), (long long)d.size(), (it & 1) != 0, &sum);
    if (rc == FV_OK) ++mut_ok;
    if (rc == -100) { fprintf(stderr, "mutation %d: malformed result\n", it); ++bad; }
  }
  printf("files %zu served %d bad %d; truncations decoded %d of %zu; mutations decoded %d of 4000; checksum %lld\n",
         files.size(), served, bad, trunc_ok, files[0].size(), mut_ok, sum);
  return bad ? 1 : 0;
}
