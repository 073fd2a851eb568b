// The row body of the cross-entropy kernels: one wave per row, the row in registers (C <= 64 * EPL), max and sums as
// wave reductions.  Shared by csrc/loss.hip (the training losses, fv_soft_target_ce / fv_label_ce) and csrc/eval.hip
// (the validation metrics, fv_eval_accumulate), so that a validation row's loss and top-1 flag cannot drift from what
// fv_label_ce writes for it.
#pragma once
#include "common.h"

namespace fv_ce_row {

constexpr int EPL = 32;      // elements per lane: rows up to 2048 classes

// Where a row's target comes from.  Both sources feed ONE row body (soft_ce_row_body), so the dense loss and the loss on
// labels cannot drift apart: fv_label_ce returns the bits fv_soft_target_ce returns on the tensor fv_mixup_target writes.
struct DenseTarget {                     // a (B, C) fp32 tensor
  static constexpr bool kHasLabel = false;
  const float* tr;
  long long label;                       // (unused)
  __device__ __forceinline__ float at(int c) const { return tr[c]; }
};

__device__ __forceinline__ float rounded(float x) {
  asm("" : "+v"(x));          // an opaque copy: the product that made it cannot be contracted into the sum that uses it
  return x;
}
// timm.data.Mixup's target at class c: fl(y1 * lam) + fl(y2 * (1 - lam)), y = on at the label, off elsewhere.  The two
// products are rounded separately, as torch's y1 * lam + y2.flip(0) * (1. - lam) rounds them (-ffast-math would fuse one
// of them into the add).
__device__ __forceinline__ float mix_target_value(int c, long long la, long long lb, float on, float off, float lam, float oml) {
#pragma clang fp reassociate(off) contract(off)
  const float y1 = c == la ? on : off, y2 = c == lb ? on : off;
  return rounded(y1 * lam) + rounded(y2 * oml);
}

template <bool MIX>
struct LabelTarget {                     // built in registers: two labels, on / off, and (MIX) the block's two weights
  static constexpr bool kHasLabel = true;
  long long label, partner;
  float on, off, lam, oml;
  // (an opaque value, like the dense source's load: the sums of the row body see the same thing from either source)
  __device__ __forceinline__ float at(int c) const {
    if constexpr (MIX) return rounded(mix_target_value(c, label, partner, on, off, lam, oml));
    else return rounded(c == label ? on : off);
  }
};

template <typename T, typename TS>
__device__ __forceinline__ void soft_ce_row_body(const T* __restrict__ xr, const TS& ts, float* __restrict__ loss_rows,
                                                 float* __restrict__ dx, int32_t* __restrict__ correct_rows, int row, int C,
                                                 float inv_b) {
  const int lane = threadIdx.x & 63;
  float xv[EPL], tv[EPL];
  float mx = -3.0e38f;
#pragma unroll
  for (int k = 0; k < EPL; ++k) {
    const int c = k * 64 + lane;
    xv[k] = c < C ? io<T>::ld(xr + c) : -3.0e38f;
    tv[k] = c < C ? ts.at(c) : 0.f;
    mx = fmaxf(mx, xv[k]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  if constexpr (TS::kHasLabel) {
    if (correct_rows) {          // top-1: the first class that attains the row maximum (torch.argmax's choice on a tie)
      int first = 0x7fffffff;
#pragma unroll
      for (int k = EPL - 1; k >= 0; --k) {
        const int c = k * 64 + lane;
        if (c < C && xv[k] == mx) first = c;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o));
      if (lane == 0) correct_rows[row] = (long long)first == ts.label ? 1 : 0;
    }
  }
  float se = 0.f, st = 0.f, stx = 0.f;
#pragma unroll
  for (int k = 0; k < EPL; ++k) {
    const int c = k * 64 + lane;
    const float e = c < C ? __expf(xv[k] - mx) : 0.f;
    se += e;
    st += tv[k];
    stx += c < C ? tv[k] * (xv[k] - mx) : 0.f;
    xv[k] = e;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    se += __shfl_xor(se, o);
    st += __shfl_xor(st, o);
    stx += __shfl_xor(stx, o);
  }
  // sum_c -t (x - mx - log se) = st * log se - sum_c t (x - mx)
  if (lane == 0) loss_rows[row] = st * __logf(se) - stx;
  if (!dx) return;
  const float rs = st / se;
  float* dr = dx + (size_t)row * C;
#pragma unroll
  for (int k = 0; k < EPL; ++k) {
    const int c = k * 64 + lane;
    if (c < C) dr[c] = (xv[k] * rs - tv[k]) * inv_b;
  }
}

}  // namespace fv_ce_row
