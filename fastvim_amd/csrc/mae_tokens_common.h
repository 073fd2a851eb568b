// What the MAE token files (mae_tokens.hip, mae_tokens_cls.hip) share: the fixed-order fp64 column sum behind the
// gradients of ``mask_token`` and ``cls_token``, the rounding "to x's type", and the entry points' argument checks.
// Both files include it BEHIND their file-scope ``#pragma clang fp reassociate(off) contract(off)``: every sum here has ONE
// order, the one written.
#pragma once
#include "common.h"
#include "rowwalk.h"

namespace {

constexpr int DT_ROWS = FV_MAE_DECODER_ROWS_PER_BLOCK;
constexpr int DT_FINAL_WAVES = 16;

// ``t.to(x.dtype).float()``: round to nearest even for bf16, the value itself for fp32
template <typename TX>
__device__ __forceinline__ float round_to_type(float t) {
  if constexpr (sizeof(TX) == 2) return bf16_bits_to_f32(f32_to_bf16_bits(t));
  else return t;
}

// A workgroup owns rows [blockIdx.x DT_ROWS, + DT_ROWS) of the rows of dout; a thread owns 4 channels of them.  A kept row
// goes to dx in x's type, a removed one -- rounded to x's type first -- into the workgroup's fp64 partial, in row order.
//   CLS = false  dout (B, L, D), dx (B, K, D): the kept row of restore index r is dx row r.
//   CLS = true   the class-token form (mae_tokens_cls.hip): dout (B, L + 1, D) with the class row LAST, dx (B, K + 1, D) with
//                the class row at K / 2 -- restore index r is dx row r + (r >= K / 2); the class row is no mask row.
template <typename TX, bool CLS>
__global__ __launch_bounds__(256) void mae_decoder_tokens_bwd_kernel(const float* __restrict__ dout, const int* __restrict__ restore,
                                                                     TX* __restrict__ dx, double* __restrict__ partials, long rows,
                                                                     int L, int K, int D) {
  constexpr int E = CLS ? 1 : 0;
  const int Lo = L + E, Kx = K + E, cls = K / 2;
  const long r0 = (long)blockIdx.x * DT_ROWS;
  const long r1 = r0 + DT_ROWS < rows ? r0 + DT_ROWS : rows;
  for (int c = threadIdx.x * 4; c < D; c += blockDim.x * 4) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (long row = r0; row < r1; ++row) {
      const long b = row / Lo;
      const int l = (int)(row - b * Lo);
      int j = -1;                         // the row of dx, wave-uniform; -1: a removed token's row
      if (CLS && l == L) {
        j = cls;
      } else {
        const int r = restore[(size_t)b * L + l];
        if (r >= 0 && r < K) j = CLS ? r + (r >= cls ? 1 : 0) : r;
      }
      float v[4];
      VecIO<float, 4>::load(dout + (size_t)row * D + c, v);
      if (j >= 0 && j < Kx) {
        VecIO<TX, 4>::store(dx + ((size_t)b * Kx + j) * D + c, v);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += (double)round_to_type<TX>(v[e]);
      }
    }
    double* dst = partials + (size_t)blockIdx.x * D + c;
#pragma unroll
    for (int e = 0; e < 4; ++e) dst[e] = acc[e];
  }
}

// A workgroup of 16 waves owns 64 channels: wave w adds partial rows w, w + 16, ... in that order, then the sixteen sums
// are added as a fixed tree.  All in fp64; one rounding, to fp32, at the end.
__global__ __launch_bounds__(64 * DT_FINAL_WAVES) void mae_decoder_tokens_final_kernel(const double* __restrict__ partials,
                                                                                       float* __restrict__ dmask_token, int nblocks,
                                                                                       int D) {
  __shared__ double s[DT_FINAL_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  double acc = 0.0;
  if (c < D) {
#pragma unroll 4
    for (int k = wave; k < nblocks; k += DT_FINAL_WAVES) acc += partials[(size_t)k * D + c];
  }
  s[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && c < D) {
    double t[DT_FINAL_WAVES];
#pragma unroll
    for (int k = 0; k < DT_FINAL_WAVES; ++k) t[k] = s[k][lane];
#pragma unroll
    for (int w = DT_FINAL_WAVES / 2; w > 0; w >>= 1) {
#pragma unroll
      for (int k = 0; k < w; ++k) t[k] = t[2 * k] + t[2 * k + 1];
    }
    dmask_token[c] = (float)t[0];
  }
}

inline bool f32_or_bf16(int dt) { return dt == FV_F32 || dt == FV_BF16; }
inline size_t esize(int dt) { return dt == FV_F32 ? 4 : 2; }
inline bool aligned_to(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }
// threads of a workgroup that walks rows with 4 channels per thread: whole waves, at most 256
inline int row_walk_threads(int dim) { return dim / 4 >= 256 ? 256 : (dim / 4 > 64 ? ((dim / 4 + 63) / 64) * 64 : 64); }

}  // namespace
