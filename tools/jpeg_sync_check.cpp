// A stand-alone program around the index-free JPEG path (include/fastvim_hip.h at ENTRIES MADE ON THE DEVICE), meant to be
// built together with fastvim_amd/csrc/jpeg_host.cpp and the two core headers fastvim_amd/csrc/jpeg_sync_core.h and
// jpeg_huff_core.h -- the text the device compiles -- by the host compiler with -fsanitize=address,undefined and run on the
// CPU (tests/test_jpeg_sync_sanitize_cpu.py):
//
//   jpeg_sync_check FILE...
//
// Every FILE the stage function takes is staged (fv_jpeg_sync_stage) with S = 1, 3 and 1000 and subsequences of 16, 64 and
// 128 bytes, for the whole image and an inner window, into a stream block of exactly the staged size and a scratch block of
// exactly the job's records; fv_jpeg_sync_host makes the entries, every fv_jpeg_huff lane of the window is run through
// the core's run_lane into a coefficient block of exactly the window's size, and the result must equal
// fv_jpeg_entropy_decode's.  Then 4000 seeded mutations of the staged scan and 4000 of the sync job's words go the same way:
// whatever they give, they must terminate without a report.  These runs are the memory-safety evidence for the device
// routine: a corrupted stream is never run on a GPU.  Exit status 0: all FILEs behaved and nothing was reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../fastvim_amd/csrc/jpeg_sync_core.h"
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

struct Staged {
  std::vector<uint8_t> pool;
  int record[FV_JPEG_REC_INTS], srec[FV_JPEG_STREAM_REC_INTS], job[FV_JPEG_SYNC_JOB_INTS];
};

// the stage into a block of exactly its size; one byte or one scratch record less is refused
int stage(const std::vector<uint8_t>& file, const int* win, int S, int L, Staged* out) {
  Exact data((long long)file.size());
  memcpy(data.p, file.data(), file.size());
  const long long big = (long long)file.size() + 16ll * win[2] * win[3] + 8192;
  Exact first(big);
  long long used = 0, rused = 0;
  int rc = fv_jpeg_sync_stage(data.p, (long long)file.size(), win, S, L, 1 << 20, first.p, big, &used, 1 << 20, &rused, 0, out->record,
                              out->srec, out->job);
  if (rc != FV_OK) return rc;
  Exact pool(used);
  long long used2 = 0, rused2 = 0;
  if (fv_jpeg_sync_stage(data.p, (long long)file.size(), win, S, L, 1 << 20, pool.p, used - 1, &used2, rused, &rused2, 0, out->record,
                         out->srec, out->job) != FV_JPEG_E_CAPACITY || used2 || rused2) return 1000;
  if (fv_jpeg_sync_stage(data.p, (long long)file.size(), win, S, L, 1 << 20, pool.p, used, &used2, rused - 1, &rused2, 0, out->record,
                         out->srec, out->job) != FV_JPEG_E_CAPACITY || used2 || rused2) return 1000;
  rc = fv_jpeg_sync_stage(data.p, (long long)file.size(), win, S, L, 1 << 20, pool.p, used, &used2, rused, &rused2, 0, out->record,
                          out->srec, out->job);
  if (rc != FV_OK || used2 != used || rused2 != rused || rused != out->job[16]) return 1001;
  out->pool.assign(pool.p, pool.p + used);
  return FV_OK;
}

// the passes, then every lane.  Returns the job's status; `statuses` counts lanes that gave up; `out` gets the coefficients.
int run(const Staged& s, const int* job, int cls, const int* win, std::vector<int16_t>* out, long long* statuses) {
  const long long used = (long long)s.pool.size();
  Exact pool(used);
  memcpy(pool.p, s.pool.data(), s.pool.size());
  const long long records = s.job[16];                      // what the stage took, whatever the (mutated) job says
  Exact scratch(records * FV_JPEG_SYNC_REC_BYTES);
  memset(scratch.p, 0xA5, (size_t)(records * FV_JPEG_SYNC_REC_BYTES));
  int j[FV_JPEG_SYNC_JOB_INTS];
  memcpy(j, job, sizeof(j));
  if (fv_jpeg_sync_host(pool.p, used, j, scratch.p, records) != FV_OK) return 1002;
  const long long n = elements(cls, win);
  Exact coef(n * 2);
  memset(coef.p, 0x5A, (size_t)(n * 2));
  const long long lanes = (long long)s.srec[9] * s.srec[5];
  for (long long lane = 0; lane < lanes; ++lane)
    if (fvhuff::run_lane(pool.p, used, s.srec, lane, (int16_t*)coef.p, n) != fvhuff::ST_OK) ++*statuses;
  if (out) out->assign((int16_t*)coef.p, (int16_t*)coef.p + n);
  return j[0] == 1 ? j[fvsync::JOB_STATUS] : 0;             // a slot without a job is left as it is, its status word too
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
  if (files.empty()) { fprintf(stderr, "usage: jpeg_sync_check FILE...\n"); return 2; }
  const int kS[3] = {1, 3, 1000}, kL[3] = {16, 64, 128};
  struct Case { Staged s; int cls; int win[4]; };
  std::vector<Case> cases;
  int staged = 0, refused = 0, bad = 0;
  long long sum = 0;
  for (size_t k = 0; k < files.size(); ++k) {
    const std::vector<uint8_t>& d = files[k];
    int info[FV_JPEG_INFO_INTS];
    if (fv_jpeg_probe(d.data(), (long long)d.size(), info) != FV_OK || !info[4]) { ++refused; continue; }
    bool counted = false;
    for (int si = 0; si < 3; ++si)
      for (int li = 0; li < 3; ++li)
        for (int inner = 0; inner < 2; ++inner) {
          Case c;
          c.cls = info[3];
          c.win[0] = 0; c.win[1] = 0; c.win[2] = info[6]; c.win[3] = info[7];
          if (inner) {
            if (info[6] < 3 || info[7] < 3) continue;
            c.win[0] = 1; c.win[1] = 1; c.win[2] = info[6] - 2; c.win[3] = info[7] - 2;
          }
          const int rc = stage(d, c.win, kS[si], kL[li], &c.s);
          if (rc == FV_JPEG_E_UNSERVED) { if (!counted) ++refused; counted = true; continue; }
          if (rc != FV_OK) { fprintf(stderr, "%s: S %d L %d window %d: stage %d\n", argv[k + 1], kS[si], kL[li], inner, rc); ++bad; continue; }
          if (!counted) ++staged;
          counted = true;
          std::vector<int16_t> got;
          long long statuses = 0;
          const int st = run(c.s, c.s.job, c.cls, c.win, &got, &statuses);
          const long long n_el = elements(c.cls, c.win);
          std::vector<int16_t> want((size_t)n_el);
          int record[FV_JPEG_REC_INTS];
          const int rc2 = fv_jpeg_entropy_decode(d.data(), (long long)d.size(), c.win, want.data(), n_el, record);
          if (st != 0 || rc2 != FV_OK || statuses || got != want || memcmp(record, c.s.record, sizeof(record))) {
            fprintf(stderr, "%s: S %d L %d window %d: status %d, host decoder %d, %lld lanes gave up, coefficients %s\n", argv[k + 1], kS[si],
                    kL[li], inner, st, rc2, statuses, got == want ? "equal" : "differ");
            ++bad;
          }
          for (int16_t v : got) sum += v;
          cases.push_back(c);
        }
  }
  if (cases.empty()) { fprintf(stderr, "no FILE could be staged\n"); return 2; }
  uint64_t state = 0x9E3779B97F4A7C15ull;
  auto next = [&state]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(state >> 33); };
  long long scan_lost = 0, scan_lanes = 0, job_skipped = 0, job_lost = 0;
  for (int it = 0; it < 8000; ++it) {
    const Case& c = cases[(size_t)next() % cases.size()];
    Staged s = c.s;
    int job[FV_JPEG_SYNC_JOB_INTS];
    memcpy(job, c.s.job, sizeof(job));
    const bool on_job = it >= 4000;
    const int edits = 1 + next() % 3;
    for (int e = 0; e < edits; ++e) {
      if (on_job) {
        // a word replaced, a byte of a word replaced, or a small step: the last two get past more of the checks
        const int w = next() % FV_JPEG_SYNC_JOB_INTS, how = next() % 3;
        if (how == 0) job[w] = (int)(next() << 1 ^ next());
        else if (how == 1) ((uint8_t*)job)[4 * w + next() % 4] = (uint8_t)next();
        else job[w] += (int)(next() % 5) - 2;
      } else {
        const long long soff = fvhuff::rec64(c.s.job, 10);
        s.pool[(size_t)(soff + next() % c.s.job[12])] = (uint8_t)next();
      }
    }
    long long statuses = 0;
    const int st = run(s, job, c.cls, c.win, nullptr, &statuses);
    if (st >= 1000) { fprintf(stderr, "mutation %d: fv_jpeg_sync_host refused its arguments (%d)\n", it, st); ++bad; }
    if (on_job) { job_skipped += st == fvsync::ST_JOB; job_lost += st == fvsync::ST_LOST; }
    else { scan_lost += st == fvsync::ST_LOST; scan_lanes += statuses != 0; }
  }
  printf("files %zu staged %d refused %d bad %d; scan mutations: %lld of 4000 lost, %lld with a lane that gave up; job mutations: "
         "%lld of 4000 skipped, %lld lost; checksum %lld\n",
         files.size(), staged, refused, bad, scan_lost, scan_lanes, job_skipped, job_lost, sum);
  return bad ? 1 : 0;
}
