// Class-token assembly of the supervised Vim baseline (fastvim_amd/vim.py with ``fused_cls``): the M patch tokens of a
// sample with the class token put in at place p (M / 2 for ``use_middle_cls_token``, else 0) and the position table
// added, one launch each way where the torch chain takes an expand, a cast, a cat of two slices and an add -- and, backward,
// slice copies and two sums over the batch.
//   vim_cls_tokens_fwd  out (B, M + 1, D) fp32 from y (B, M, D) in T (fp32 or bf16): row j is
//                       (j == p ? cls_token rounded to T : y[b, j - (j > p)]) + pos_embed[j] -- ONE fp32 add, what
//                       ``cat(...) + pos_embed`` evaluates (a bf16 y promotes to fp32 against the fp32 table).
//                       A thread moves 4 channels (8 for bf16 when D % 8 == 0): 16 bytes of y.
//   vim_cls_tokens_bwd  from dout (B, M + 1, D) fp32: dy[b, i] = dout[b, i + (i >= p)] rounded to T (fp32: the bits move);
//                       d pos_embed[j, d] the sum over b = 0 .. B-1 of dout[b, j, d], in fp64 in that order, rounded once
//                       to fp32; d cls_token[d] the same sum of row p with every term rounded to T first (fp32: it IS
//                       d pos_embed[p, d]).  One thread per (row j, VEC channels) walks the batch: all three results in
//                       one launch, no partial buffer, no second pass over dout.
// No atomics, nothing that waits for the host.  Floating-point reassociation and contraction are switched off for the whole
// file: every sum has ONE order, the one written.
#include "common.h"
#include "rowwalk.h"

#pragma clang fp reassociate(off) contract(off)

#include "mae_tokens_common.h"      // round_to_type, the argument checks (behind the pragma)

namespace {

template <typename T, int VEC>
__global__ __launch_bounds__(256) void vim_cls_tokens_fwd_kernel(const T* __restrict__ y, const float* __restrict__ cls_token,
                                                                 const float* __restrict__ pos, float* __restrict__ out,
                                                                 long units, int M, int D, int p) {
  const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= units) return;
  const int upr = D / VEC;
  const long row = u / upr;               // b * (M + 1) + j
  const int c = (int)(u - row * upr) * VEC;
  const long b = row / (M + 1);
  const int j = (int)(row - b * (M + 1));
  float v[VEC], pe[VEC];
  if (j == p) {                           // cls_token.expand(B, -1, -1).to(x.dtype)
    VecIO<float, VEC>::load(cls_token + c, v);
#pragma unroll
    for (int e = 0; e < VEC; ++e) v[e] = round_to_type<T>(v[e]);
  } else {
    VecIO<T, VEC>::load(y + ((size_t)b * M + (j - (j > p ? 1 : 0))) * D + c, v);
  }
  VecIO<float, VEC>::load(pos + (size_t)j * D + c, pe);
#pragma unroll
  for (int e = 0; e < VEC; ++e) v[e] = v[e] + pe[e];
  VecIO<float, VEC>::store(out + (size_t)row * D + c, v);
}

// One thread per (row j of the M + 1, VEC channels); the batch is walked in order, UNR samples' loads in flight.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void vim_cls_tokens_bwd_kernel(const float* __restrict__ dout, T* __restrict__ dy,
                                                                 float* __restrict__ dpos, float* __restrict__ dcls, int units,
                                                                 int B, int M, int D, int p) {
  constexpr int UNR = 4;
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= units) return;
  const int upr = D / VEC;
  const int j = u / upr;                  // 0 .. M
  const int c = (u - j * upr) * VEC;
  const bool is_cls = j == p;
  const size_t in_stride = (size_t)(M + 1) * D, out_stride = (size_t)M * D;
  const float* src = dout + (size_t)j * D + c;
  T* dst = dy + (size_t)(is_cls ? 0 : j - (j > p ? 1 : 0)) * D + c;      // (never written for the class row)
  double acc[VEC], acc_cls[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) acc[e] = acc_cls[e] = 0.0;
  int b = 0;
  for (; b + UNR <= B; b += UNR) {
    float v[UNR][VEC];
#pragma unroll
    for (int k = 0; k < UNR; ++k) VecIO<float, VEC>::load(src + (size_t)(b + k) * in_stride, v[k]);
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
      if (!is_cls) VecIO<T, VEC>::store(dst + (size_t)(b + k) * out_stride, v[k]);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        acc[e] += (double)v[k][e];
        acc_cls[e] += (double)round_to_type<T>(v[k][e]);
      }
    }
  }
  for (; b < B; ++b) {
    float v[VEC];
    VecIO<float, VEC>::load(src + (size_t)b * in_stride, v);
    if (!is_cls) VecIO<T, VEC>::store(dst + (size_t)b * out_stride, v);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      acc[e] += (double)v[e];
      acc_cls[e] += (double)round_to_type<T>(v[e]);
    }
  }
  float o[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) o[e] = (float)acc[e];
  VecIO<float, VEC>::store(dpos + (size_t)j * D + c, o);
  if (is_cls) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) o[e] = (float)acc_cls[e];
    VecIO<float, VEC>::store(dcls + c, o);
  }
}

int vim_check(const char* who, const void* a, const void* b, const void* c, const void* d, int y_dtype, int batch, int len,
              int dim, int position) {
  FV_CHECK(a && b && c && d, "%s: null pointer", who);
  FV_CHECK(batch > 0 && len > 0 && dim > 0, "%s: empty dimension", who);
  FV_CHECK(position >= 0 && position <= len, "%s: the class position %d is not in 0 .. %d", who, position, len);
  FV_CHECK(dim % 4 == 0, "%s: dim %d must be a multiple of 4", who, dim);
  FV_CHECK(f32_or_bf16(y_dtype), "%s: y must be fp32 or bf16", who);
  FV_CHECK((long)batch * ((long)len + 1) <= 0x7fffffffL, "%s: too many rows", who);
  FV_CHECK(((long)len + 1) * (dim / 4) <= 0x7fffffffL, "%s: too many elements per sample", who);
  FV_CHECK((long)batch * ((long)len + 1) * (dim / 4) <= (1L << 38), "%s: too many elements for one launch", who);
  return FV_OK;
}

}  // namespace

extern "C" int fv_vim_cls_tokens_fwd(const void* y, int y_dtype, const float* cls_token, const float* pos_embed, float* out,
                                     int batch, int len, int dim, int position, fv_stream_t stream) {
  const int rc = vim_check("vim_cls_tokens_fwd", y, cls_token, pos_embed, out, y_dtype, batch, len, dim, position);
  if (rc != FV_OK) return rc;
  FV_CHECK(aligned_to(y, esize(y_dtype)) && aligned_to(cls_token, 4) && aligned_to(pos_embed, 4) && aligned_to(out, 4),
           "vim_cls_tokens_fwd: a buffer is not aligned to its element size");
  hipStream_t st = (hipStream_t)stream;
  const bool wide = y_dtype == FV_BF16 && dim % 8 == 0;
  const long units = (long)batch * (len + 1) * (dim / (wide ? 8 : 4));
  const dim3 grid(fv_cdiv(units, 256)), block(256);
#define FV_VT(T, VEC) hipLaunchKernelGGL((vim_cls_tokens_fwd_kernel<T, VEC>), grid, block, 0, st, (const T*)y, cls_token, pos_embed, out, units, len, dim, position)
  if (wide) FV_VT(bf16_t, 8);
  else if (y_dtype == FV_BF16) FV_VT(bf16_t, 4);
  else FV_VT(float, 4);
#undef FV_VT
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_vim_cls_tokens_bwd(const float* dout, void* dy, int y_dtype, float* dpos_embed, float* dcls_token, int batch,
                                     int len, int dim, int position, fv_stream_t stream) {
  const int rc = vim_check("vim_cls_tokens_bwd", dout, dy, dpos_embed, dcls_token, y_dtype, batch, len, dim, position);
  if (rc != FV_OK) return rc;
  FV_CHECK(aligned_to(dout, 4) && aligned_to(dy, esize(y_dtype)) && aligned_to(dpos_embed, 4) && aligned_to(dcls_token, 4),
           "vim_cls_tokens_bwd: a buffer is not aligned to its element size");
  hipStream_t st = (hipStream_t)stream;
  const bool wide = y_dtype == FV_BF16 && dim % 8 == 0;
  const int units = (len + 1) * (dim / (wide ? 8 : 4));
  const dim3 grid(fv_cdiv(units, 64)), block(64);      // one wave a workgroup: (M + 1) D / 4 threads are few, spread them
#define FV_VT(T, VEC) hipLaunchKernelGGL((vim_cls_tokens_bwd_kernel<T, VEC>), grid, block, 0, st, dout, (T*)dy, dpos_embed, dcls_token, units, batch, len, dim, position)
  if (wide) FV_VT(bf16_t, 8);
  else if (y_dtype == FV_BF16) FV_VT(bf16_t, 4);
  else FV_VT(float, 4);
#undef FV_VT
  FV_LAUNCH_CHECK();
  return FV_OK;
}
