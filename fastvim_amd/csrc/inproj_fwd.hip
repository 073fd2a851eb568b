// in_proj forward of the d_model = 192 mixer: C (M, N) bf16 = A (M, 192) bf16 @ W^T, W (N, 192), N a multiple of 384, with W
// given as its fragment-major copy (fv_pack_weight_frags_in_batched; fastvim_amd.mixer_ops.pack_index_in).
// One workgroup of four waves owns a tile of up to 64 rows with the whole K: the 24 KB tile goes to LDS once (rows 400 bytes
// apart: fragment reads conflict-free), and tile_times_packed_w (gemm_tiles.h) multiplies it by the weight, which every wave
// streams from L2 straight into MFMA operand registers for its 96 columns of each 384-column pass -- the second phase of
// fv_mixer_conv_pool_bwd_dgrad_pk2 with a K-contiguous weight and N / 384 passes.  Against the 160 x 128 tiles of
// fv_gemm_bf16 at this shape: A is read once instead of six times, no LDS weight stage, no barrier and no vmcnt(0) in the
// K loop, and a pass's C stores run under the next pass's loop.  Bit-identical to fv_gemm_bf16.
#include "gemm_tiles.h"

namespace {

constexpr int IP_K = TPW_K, IP_BM = 64, IP_NT = 256;
constexpr int IP_RS = IP_K * 2 + 16;                       // tile row stride (bytes): = 4 dwords (mod 32) per row, as CD_RSB
constexpr int IP_O_SLAB = IP_BM * IP_RS, IP_SMEM = IP_O_SLAB + 4 * TPW_SLAB;      // 25 600 + 13 312
constexpr int IP_UPR = IP_K / 8, IP_NV = IP_BM * IP_UPR / IP_NT;                  // 16-byte units per row, per thread (6)
static_assert(IP_BM * IP_UPR % IP_NT == 0 && TPW_SLAB % 16 == 0 && IP_O_SLAB % 16 == 0, "tile staging");

// rpt: rows of C a workgroup owns (1..64); tile rows past them (and past M) are zero in LDS and never stored
__global__ __launch_bounds__(IP_NT, 2) void inproj_fwd_pk_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ Wpk,
                                                                  bf16_t* __restrict__ C, int M, int N, int rpt) {
  __shared__ __attribute__((aligned(16))) char smem[IP_SMEM];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long m0 = (long)blockIdx.x * rpt;
  const int live = (int)min((long)rpt, (long)M - m0);
  // the tile's rows are one contiguous run of A (lda == 192): 16-byte loads, six per thread, in flight together
  u32x4 av[IP_NV];
  const u32x4* a16 = reinterpret_cast<const u32x4*>(A + m0 * IP_K);
#pragma unroll
  for (int i = 0; i < IP_NV; ++i) {
    const int u = tid + i * IP_NT;
    av[i] = u < live * IP_UPR ? a16[u] : (u32x4){0u, 0u, 0u, 0u};
  }
  TpwRing ring;
  ring.prefill(Wpk, wv, lane);      // the first three k steps of the weight arrive under the tile's trip through LDS
#pragma unroll
  for (int i = 0; i < IP_NV; ++i) {
    const int u = tid + i * IP_NT, r = u / IP_UPR, c = u - r * IP_UPR;
    *reinterpret_cast<u32x4*>(smem + r * IP_RS + c * 16) = av[i];
  }
  __syncthreads();
  // two passes per call (N = 768 is one call): inside a call the weight ring runs through the pass boundary
  auto rowof = [m0, live](int r) { return r < live ? m0 + r : -1L; };
  char* slab = smem + IP_O_SLAB + wv * TPW_SLAB;
  const int npass = N / 384;
  int p0 = 0;
  for (; p0 + 2 <= npass; p0 += 2) {
    if (p0) ring.prefill(Wpk, wv, lane, p0);
    tile_times_packed_w<IP_RS, 2>(smem, slab, ring, p0, C, (long)N, rowof, wv, lane);
  }
  if (p0 < npass) {
    if (p0) ring.prefill(Wpk, wv, lane, p0);
    tile_times_packed_w<IP_RS, 1>(smem, slab, ring, p0, C, (long)N, rowof, wv, lane);
  }
}

}  // namespace

// Rows per workgroup when the caller leaves the choice to the library (rows_per_tile = 0): full 64-row tiles.  Dealing the rows
// evenly over whole rounds of resident workgroups (M = 25 088: 512 x 49 instead of 392 x 64) was measured and lost, 15.20
// against 14.45 us per launch stand-alone (profiles/inproj_pk_gate.log): every workgroup streams the whole weight and issues
// all 64 rows of MFMAs whatever its height -- the finding fused_rpt (gemm_mfma.hip) records for the fused launches.
static int ip_default_rpt(int M) {
  (void)M;
  return IP_BM;
}

// C (M, N) bf16 contiguous = A (M, 192) bf16 @ W^T with W_pk the fragment-major copy of W (N, 192) made by
// fv_pack_weight_frags_in_batched.  rows_per_tile: 0 = the library's choice, 1..64 = that many rows per workgroup, -1 = the
// rows dealt evenly over whole rounds of 2 x CU-count workgroups (M = 25 088 on 256 CUs: 512 x 49).
extern "C" int fv_gemm_bf16_inproj_pk(const void* A, const void* W_pk, void* C, int M, int N, int K, long lda,
                                      int rows_per_tile, fv_stream_t stream) {
  FV_CHECK(A && W_pk && C, "gemm_bf16_inproj_pk: null pointer");
  FV_CHECK(M > 0 && K == IP_K && N > 0 && N % 384 == 0, "gemm_bf16_inproj_pk: built for K = 192 and N a multiple of 384 (K = %d, N = %d)", K, N);
  FV_CHECK(lda == IP_K, "gemm_bf16_inproj_pk: A must be contiguous (lda = %ld, K = %d)", lda, K);
  FV_CHECK(((uintptr_t)A & 15) == 0 && ((uintptr_t)W_pk & 15) == 0 && ((uintptr_t)C & 15) == 0,
           "gemm_bf16_inproj_pk: operands must be 16-byte aligned");
  FV_CHECK(rows_per_tile >= -1 && rows_per_tile <= IP_BM, "gemm_bf16_inproj_pk: rows_per_tile must be -1, 0 or 1..%d", IP_BM);
  int rpt = rows_per_tile;
  if (rpt == 0) rpt = ip_default_rpt(M);
  if (rpt < 0) {
    const long slots = 2L * fv_cu_count(), rounds = (M + IP_BM * slots - 1) / (IP_BM * slots);
    rpt = (int)((M + slots * rounds - 1) / (slots * rounds));
    rpt = rpt < 16 ? 16 : rpt > IP_BM ? IP_BM : rpt;
  }
  hipLaunchKernelGGL(inproj_fwd_pk_kernel, dim3(fv_cdiv(M, rpt)), dim3(IP_NT), 0, (hipStream_t)stream, (const bf16_t*)A,
                     (const bf16_t*)W_pk, (bf16_t*)C, M, N, rpt);
  FV_LAUNCH_CHECK();
  return FV_OK;
}
