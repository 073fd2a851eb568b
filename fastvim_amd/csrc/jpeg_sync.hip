// hipcc-flags: -fwrapv
// fv_jpeg_sync (include/fastvim_hip.h at ENTRIES MADE ON THE DEVICE), in front of fv_jpeg_huff: the index entries of a
// JPEG file's groups found on the device, by self-synchronisation of the Huffman stream.  The decoder is
// jpeg_sync_core.h, the same text fv_jpeg_sync_host runs serially on the CPU.
//
//   jpeg_sync_kernel  ONE WORKGROUP PER SAMPLE (SYNC_THREADS lanes), the grid is `batch`: a slot without a job returns at
//                     once, and a captured launch serves whatever the job table holds when it runs.
//     1. the four Huffman tables go into LDS (5696 bytes)
//     2. speculative pass: lane t decodes subsequences t, t + T, ... each from (its first bit, b = 0, k = 0)
//     3. fixed point: per round every subsequence takes its predecessor's exit state as its entry state (first half) and
//        is decoded again if that changed it (second half); a barrier between the halves, so a round reads only what the
//        round before wrote.  An INVALID exit state is not taken (jpeg_sync_core.h at round_take).  The loop ends when a round changes nothing or after `nsub` rounds; the condition is an LDS
//        word read behind a barrier, the same value in every lane.
//     4. scan: each lane sums a contiguous share of the records, a workgroup scan over the lanes' sums in LDS, and each
//        lane writes the first MCU start and the entry predictors of its records; the same scan joins the MCU starts in
//        front of the first INVALID exit state, which decide the status
//     5. emission: lane t walks subsequences t, t + T, ... from their final entry states and writes the 16-byte entry of
//        every group start the window needs where fv_jpeg_huff reads it
//   The states live in a global scratch buffer, 32 bytes per subsequence, sized by the stage's capacity; the stream bytes
//   are read from the pool through the caches.
//
// REQUIREMENTS this kernel keeps:
//   * Every lane of a workgroup reaches every barrier: the only branches and loops around a barrier depend on the job's
//     words, on blockIdx, or on an LDS word read behind a barrier -- the same in every lane.  No barrier sits inside a
//     per-lane loop.
//   * Every loop bound comes from the job's byte and subsequence counts, which the host capped (open_job checks them
//     again): `nsub` rounds, ceil(nsub / T) subsequences per lane and pass, 8 * bytes + 8 symbols per subsequence.
//   * Every table, stream and state access is range-checked: open_job holds the job's offsets and counts against the pool's
//     and the scratch buffer's size, the core holds every stream read against the staged scan.  A job that does not fit is
//     skipped with FV_JPEG_ST_SYNC_JOB.
//   * Plain vector stores only; no atomics.  Every record and every entry is written by exactly one lane between two
//     barriers; the round's flag is an LDS word every lane that sets it sets to 1.
//   * A sample whose fixed point turns INVALID before the last group start the window needs writes FV_JPEG_ST_SYNC_LOST
//     and no entries: the reserved entries stay as the host filled them, and fv_jpeg_huff's lanes give FV_JPEG_ST_RECORD.
#include "common.h"
#include "jpeg_sync_core.h"

namespace {

constexpr int SYNC_THREADS = 256;
constexpr int TABLE_WORDS4 = fvhuff::TABLES * fvhuff::TABLE_WORDS;
static_assert(FV_JPEG_SYNC_JOB_INTS == fvsync::JOB_INTS && FV_JPEG_ST_SYNC_JOB == fvsync::ST_JOB && FV_JPEG_ST_SYNC_LOST == fvsync::ST_LOST &&
              FV_JPEG_SYNC_REC_BYTES == 4 * fvsync::REC_WORDS, "the sync core and the header agree");

__global__ __launch_bounds__(SYNC_THREADS) void jpeg_sync_kernel(uint8_t* pool, long long pool_bytes, int* jobs, uint32_t* scratch,
                                                                  long long scratch_records, int batch) {
  __shared__ uint32_t s_tables[TABLE_WORDS4];
  __shared__ uint32_t s_scan[4][SYNC_THREADS];
  __shared__ uint32_t s_valid[2][SYNC_THREADS];              // fvsync::Prefix of the lanes' shares
  __shared__ int s_flag;
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= batch) return;
  int* j = jobs + (long long)blockIdx.x * fvsync::JOB_INTS;
  if (j[0] != 1) return;                                      // no job in this slot
  fvsync::Job J;
  if (!fvsync::open_job(j, pool_bytes, scratch_records, J)) {      // the job's words: the same verdict in every lane
    if (tid == 0) j[fvsync::JOB_STATUS] = fvsync::ST_JOB;
    return;
  }
  const uint32_t* gt = reinterpret_cast<const uint32_t*>(pool + J.toff);
  for (int w = tid; w < TABLE_WORDS4; w += SYNC_THREADS) s_tables[w] = gt[w];
  __syncthreads();
  const uint32_t* tables = s_tables;
  const uint8_t* d = pool + J.soff;
  uint32_t* recs = scratch + J.roff * fvsync::REC_WORDS;
  const uint32_t nsub = J.nsub;

  for (uint32_t i = tid; i < nsub; i += SYNC_THREADS) fvsync::pass_speculate(J, d, tables, recs, i);

  int rounds = 0;
  for (uint32_t r = 0; r < nsub; ++r) {
    if (tid == 0) s_flag = 0;
    __syncthreads();                                          // the exit states of the round before are written
    bool any = false;
    for (uint32_t i = tid; i < nsub; i += SYNC_THREADS) any |= fvsync::round_take(recs, i);
    if (any) s_flag = 1;
    __syncthreads();
    const int changed = s_flag;
    __syncthreads();                                          // everybody has read the flag before it is reset
    if (!changed) break;
    for (uint32_t i = tid; i < nsub; i += SYNC_THREADS) fvsync::round_decode(J, d, tables, recs, i);
    ++rounds;
  }
  __syncthreads();

  // the scan: a contiguous share of the records per lane
  const uint32_t share = (nsub + SYNC_THREADS - 1) / SYNC_THREADS;
  const uint32_t c0 = (uint32_t)tid * share < nsub ? (uint32_t)tid * share : nsub, c1 = c0 + share < nsub ? c0 + share : nsub;
  uint32_t mine[4] = {0, 0, 0, 0};
  fvsync::Prefix valid{0u, 0u};
  for (uint32_t i = c0; i < c1; ++i) {
    const uint32_t* rec = recs + (size_t)i * fvsync::REC_WORDS;
    valid = fvsync::join(valid, fvsync::prefix_of(rec));
    mine[0] += rec[4]; mine[1] += rec[5] & 0xffffu; mine[2] += rec[5] >> 16; mine[3] += rec[6] & 0xffffu;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) s_scan[q][tid] = mine[q];
  s_valid[0][tid] = valid.n;
  s_valid[1][tid] = valid.dead;
  __syncthreads();
  for (int off = 1; off < SYNC_THREADS; off <<= 1) {
    uint32_t v[4] = {0, 0, 0, 0};
    fvsync::Prefix before{0u, 0u};
    if (tid >= off) {
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = s_scan[q][tid - off];
      before = fvsync::Prefix{s_valid[0][tid - off], s_valid[1][tid - off]};
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) s_scan[q][tid] += v[q];
    valid = fvsync::join(before, valid);                    // the lanes in front come first: the join is not commutative
    s_valid[0][tid] = valid.n;
    s_valid[1][tid] = valid.dead;
    __syncthreads();
  }
  uint32_t run[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) run[q] = s_scan[q][tid] - mine[q];      // exclusive
  const uint32_t total = s_scan[0][SYNC_THREADS - 1];
  for (uint32_t i = c0; i < c1; ++i) {
    uint32_t* rec = recs + (size_t)i * fvsync::REC_WORDS;
    const uint32_t n = rec[4], s01 = rec[5], s2 = rec[6];
    rec[4] = run[0];
    rec[5] = (run[1] & 0xffffu) | (run[2] & 0xffffu) << 16;
    rec[6] = run[3] & 0xffffu;
    run[0] += n; run[1] += s01 & 0xffffu; run[2] += s01 >> 16; run[3] += s2 & 0xffffu;
  }
  __syncthreads();

  // the MCU starts in front of the first INVALID exit state; an LDS word behind a barrier: uniform
  const bool lost = (long long)s_valid[0][SYNC_THREADS - 1] <= fvsync::last_needed(J);
  if (tid == 0) {
    j[fvsync::JOB_ROUNDS] = rounds;
    j[fvsync::JOB_STATUS] = lost ? fvsync::ST_LOST : 0;
  }
  if (lost) return;
  for (uint32_t i = tid; i < nsub; i += SYNC_THREADS)
    fvsync::pass_emit(J, d, tables, recs, i, i + 1 < nsub ? recs[(size_t)(i + 1) * fvsync::REC_WORDS + 4] : total, pool);
}

bool batch_ok(int batch) { return batch >= 1 && batch <= 4096; }

}  // namespace

extern "C" long long fv_jpeg_sync_table_ints(int batch) { return batch_ok(batch) ? (long long)batch * FV_JPEG_SYNC_JOB_INTS : 0; }

extern "C" int fv_jpeg_sync(void* stream_pool, long long stream_bytes, int* sync_table, void* scratch, long long scratch_bytes,
                            int batch, fv_stream_t stream) {
  FV_CHECK(stream_pool && sync_table && scratch, "jpeg_sync: null pointer");
  FV_CHECK(batch_ok(batch), "jpeg_sync: batch %d outside [1, 4096]", batch);
  FV_CHECK(stream_bytes >= 0 && scratch_bytes >= 0, "jpeg_sync: negative capacity");
  FV_CHECK(((uintptr_t)stream_pool & 15) == 0 && ((uintptr_t)sync_table & 3) == 0 && ((uintptr_t)scratch & 15) == 0,
           "jpeg_sync: misaligned buffer (stream pool and scratch 16 bytes, table 4)");
  hipLaunchKernelGGL(jpeg_sync_kernel, dim3(batch), dim3(SYNC_THREADS), 0, (hipStream_t)stream, (uint8_t*)stream_pool, stream_bytes,
                     sync_table, (uint32_t*)scratch, scratch_bytes / FV_JPEG_SYNC_REC_BYTES, batch);
  FV_LAUNCH_CHECK();
  return FV_OK;
}
