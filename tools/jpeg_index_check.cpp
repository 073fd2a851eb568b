// A stand-alone program around the JPEG index (include/fastvim_hip.h at THE INDEX), meant to be built together with
// fastvim_amd/csrc/jpeg_host.cpp and the decode core fastvim_amd/csrc/jpeg_huff_core.h -- the text the device compiles -- by
// the host compiler with -fsanitize=address,undefined and run on the CPU (tests/test_jpeg_index_sanitize_cpu.py):
//
//   jpeg_index_check FILE...
//
// Every served FILE without a restart interval is indexed with S = 1, 2, 3, 8 and 1000; for the whole image and an inner
// window the index is staged (fv_jpeg_index_stage) and every lane of the window is run through the core's run_lane, as the
// kernel runs it, into a coefficient block of exactly the window's size out of a stream block of exactly the staged size;
// the result must equal fv_jpeg_entropy_decode's.  Then 4000 seeded mutations of the file's scan with the index kept and
// 4000 mutations of the index with the file kept go the same way (host checks, then every lane): whatever they decode,
// they must terminate without a report.  These runs are the memory-safety evidence for the device routine: a corrupted
// stream is never run on a GPU.  Exit status 0: all FILEs behaved and nothing was reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../fastvim_amd/csrc/jpeg_huff_core.h"
#include "../include/fastvim_hip.h"

namespace {

long long elements(int cls, const int* win) {
  const long long per = cls == FV_JPEG_GRAY ? 1 : cls == FV_JPEG_444 ? 3 : cls == FV_JPEG_422 ? 4 : 6;
  return (long long)win[2] * win[3] * per * 64;
}

struct Exact {      // a heap block of exactly n bytes (at least 1 for malloc), 16-byte aligned by malloc
  uint8_t* p;
  explicit Exact(long long n) : p((uint8_t*)malloc(n > 0 ? (size_t)n : 1)) {}
  ~Exact() { free(p); }
};

// stage + every lane.  Returns the stage's code; `statuses` counts lanes that gave up; `out` gets the coefficients.
int run(const std::vector<uint8_t>& file, const std::vector<uint8_t>& index, const int* win, int cls, int verify,
        std::vector<int16_t>* out, long long* statuses) {
  Exact data((long long)file.size()), idx((long long)index.size());
  memcpy(data.p, file.data(), file.size());
  memcpy(idx.p, index.data(), index.size());
  const long long big = (long long)file.size() + (long long)index.size() + 8192;
  Exact scratch(big);
  int record[FV_JPEG_REC_INTS], srec[FV_JPEG_STREAM_REC_INTS];
  long long used = 0;
  int rc = fv_jpeg_index_stage(data.p, (long long)file.size(), idx.p, (long long)index.size(), win, verify, scratch.p, big, &used, 0,
                               record, srec);
  if (rc != FV_OK) return rc;
  // one byte less is refused, the exact size is taken
  long long used2 = 0;
  Exact pool(used);
  if (fv_jpeg_index_stage(data.p, (long long)file.size(), idx.p, (long long)index.size(), win, verify, pool.p, used - 1, &used2, 0,
                          record, srec) != FV_JPEG_E_CAPACITY) return 1000;
  used2 = 0;
  rc = fv_jpeg_index_stage(data.p, (long long)file.size(), idx.p, (long long)index.size(), win, verify, pool.p, used, &used2, 0, record,
                           srec);
  if (rc != FV_OK || used2 != used) return 1001;
  const long long n = elements(cls, win);
  Exact coef(n * 2);
  memset(coef.p, 0x5A, (size_t)(n * 2));
  const long long lanes = (long long)srec[9] * srec[5];
  for (long long lane = 0; lane < lanes; ++lane)
    if (fvhuff::run_lane(pool.p, used, srec, lane, (int16_t*)coef.p, n) != fvhuff::ST_OK) ++*statuses;
  // a lane past the last one, and a record with a field off, touch nothing
  if (fvhuff::run_lane(pool.p, used, srec, lanes, (int16_t*)coef.p, n) != fvhuff::ST_RECORD) return 1002;
  if (out) out->assign((int16_t*)coef.p, (int16_t*)coef.p + n);
  return FV_OK;
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
  if (files.empty()) { fprintf(stderr, "usage: jpeg_index_check FILE...\n"); return 2; }
  const int kS[5] = {1, 2, 3, 8, 1000};
  struct Case { size_t file; std::vector<uint8_t> index; int info[FV_JPEG_INFO_INTS]; long long scan; };
  std::vector<Case> cases;
  int indexed = 0, unindexed = 0, bad = 0;
  long long sum = 0;
  for (size_t k = 0; k < files.size(); ++k) {
    const std::vector<uint8_t>& d = files[k];
    int info[FV_JPEG_INFO_INTS];
    if (fv_jpeg_probe(d.data(), (long long)d.size(), info) != FV_OK || !info[4]) { ++unindexed; continue; }
    bool counted = false;
    for (int si = 0; si < 5; ++si) {
      const long long bound = fv_jpeg_index_bound(info[6], info[7], kS[si]);
      Exact out(bound);
      const long long n = fv_jpeg_build_index(d.data(), (long long)d.size(), kS[si], out.p, bound);
      if (n == FV_JPEG_E_UNSERVED) { if (!counted) ++unindexed; counted = true; continue; }
      if (n != bound) { fprintf(stderr, "%s: S %d: build_index gave %lld, bound %lld\n", argv[k + 1], kS[si], n, bound); ++bad; continue; }
      if (fv_jpeg_build_index(d.data(), (long long)d.size(), kS[si], out.p, bound - 1) != FV_JPEG_E_CAPACITY) { fprintf(stderr, "%s: short index capacity accepted\n", argv[k + 1]); ++bad; }
      if (!counted) ++indexed;
      counted = true;
      Case c;
      c.file = k;
      c.index.assign(out.p, out.p + n);
      memcpy(c.info, info, sizeof(info));
      uint32_t scan;
      memcpy(&scan, out.p + 64, 4);
      c.scan = scan;
      for (int inner = 0; inner < 2; ++inner) {
        int win[4] = {0, 0, info[6], info[7]};
        if (inner) {
          if (info[6] < 3 || info[7] < 3) continue;
          win[0] = 1; win[1] = 1; win[2] = info[6] - 2; win[3] = info[7] - 2;
        }
        std::vector<int16_t> got;
        long long statuses = 0;
        const int rc = run(d, c.index, win, info[3], 1, &got, &statuses);
        const long long n_el = elements(info[3], win);
        std::vector<int16_t> want((size_t)n_el);
        int record[FV_JPEG_REC_INTS];
        const int rc2 = fv_jpeg_entropy_decode(d.data(), (long long)d.size(), win, want.data(), n_el, record);
        if (rc != FV_OK || rc2 != FV_OK || statuses || got != want) {
          fprintf(stderr, "%s: S %d window %d: stage %d, host decoder %d, %lld lanes gave up, coefficients %s\n", argv[k + 1], kS[si],
                  inner, rc, rc2, statuses, got == want ? "equal" : "differ");
          ++bad;
        }
        for (int16_t v : got) sum += v;
      }
      cases.push_back(c);
    }
  }
  if (cases.empty()) { fprintf(stderr, "no FILE could be indexed\n"); return 2; }
  uint64_t state = 0x9E3779B97F4A7C15ull;
  auto next = [&state]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(state >> 33); };
  long long stream_staged = 0, stream_gave_up = 0, index_staged = 0, index_gave_up = 0;
  for (int it = 0; it < 8000; ++it) {
    const Case& c = cases[it % cases.size()];
    std::vector<uint8_t> d = files[c.file], ix = c.index;
    const bool on_index = it >= 4000;
    const int edits = 1 + next() % 3;
    for (int e = 0; e < edits; ++e) {
      if (on_index) {
        // half of the edits go to the entries and the header words, where a mutation gets past the format check
        const size_t span = (next() & 1) ? ix.size() : ix.size() - FV_JPEG_INDEX_HEAD_BYTES;
        ix[ix.size() - 1 - next() % span] = (uint8_t)next();
      } else {
        d[(size_t)c.scan + next() % (d.size() - (size_t)c.scan)] = (uint8_t)next();
      }
    }
    int win[4] = {0, 0, c.info[6], c.info[7]};
    if ((it & 1) && c.info[6] > 2 && c.info[7] > 2) { win[0] = 1; win[1] = 1; win[2] = c.info[6] - 2; win[3] = c.info[7] - 2; }
    long long statuses = 0;
    const int rc = run(d, ix, win, c.info[3], 0, nullptr, &statuses);
    if (rc >= 1000) { fprintf(stderr, "mutation %d: the exact-size stage or the lane bound misbehaved (%d)\n", it, rc); ++bad; }
    if (rc == FV_OK) ++(on_index ? index_staged : stream_staged);
    if (statuses) ++(on_index ? index_gave_up : stream_gave_up);
  }
  printf("files %zu indexed %d unindexed %d bad %d; stream mutations staged %lld of 4000, %lld with a lane that gave up; index "
         "mutations staged %lld of 4000, %lld with a lane that gave up; checksum %lld\n",
         files.size(), indexed, unindexed, bad, stream_staged, stream_gave_up, index_staged, index_gave_up, sum);
  return bad ? 1 : 0;
}
