// Token assembly of the Vim MAE baseline (fastvim_amd/fastvim_mae.py with ``fused_tokens`` or a sampler): the masked
// autoencoder whose encoder carries a class token in the MIDDLE of the K kept tokens (place c = K / 2) and whose decoder
// carries it at the END of the L grid tokens.  The plan is the one of mae_tokens.hip (keep_index, restore_index); these are
// the row copies around it, one launch each way where the torch chain takes a gather, an add, a cast and a cat (encoder)
// and two cats, a repeat, a gather and two adds (decoder).
//   mae_encoder_tokens_cls_fwd  out (B, K + 1, D) from the UN-gathered x (B, L, D): row j < c is x[b, keep[b, j]], row c is
//                               cls_token + pos[0] (added in fp32, rounded once to x's type), row j > c is x[b, keep[b, j - 1]].
//                               The copies move bits; a thread moves 4 channels (8 for bf16 when D % 8 == 0): 16 bytes.
//   mae_encoder_tokens_cls_bwd  dx (B, L, D): a kept row l takes dout[b, r + (r >= c)], r = restore[b, l]; a removed row
//                               takes zero -- every row is written, no fill pass.  mae_cls_grad: d cls_token[d] is the sum
//                               over b = 0 .. B-1 of dout[b, c, d], in fp64 in that order, rounded once to fp32.
//   mae_decoder_tokens_cls_fwd  out (B, L + 1, D) fp32 from x (B, K + 1, D): row l < L is (r >= 0 ? x[b, r + (r >= c)] :
//                               mask_token rounded to x's type) + pos[1 + l]; row L is x[b, c] + pos[0].
//   backward of the decoder     mae_decoder_tokens_bwd_kernel<., true> and mae_decoder_tokens_final_kernel of
//                               mae_tokens_common.h: the kernels of the class-token-free decoder, told where the class rows are.
// No atomics, nothing that waits for the host.  Every index read from memory is checked against its range before it is used.
// Floating-point reassociation and contraction are switched off for the whole file: every sum has ONE order, the one written.
#include "common.h"
#include "rowwalk.h"

#pragma clang fp reassociate(off) contract(off)

#include "mae_tokens_common.h"      // (behind the pragma)

namespace {

// ---- encoder input.  One thread per (output row, VEC channels); T in and out.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void mae_encoder_tokens_cls_fwd_kernel(const T* __restrict__ x, const float* __restrict__ cls_token,
                                                                         const float* __restrict__ pos, const int* __restrict__ keep,
                                                                         T* __restrict__ out, long units, int L, int K, int D) {
  const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= units) return;
  const int upr = D / VEC;
  const long row = u / upr;               // b * (K + 1) + j
  const int c = (int)(u - row * upr) * VEC;
  const long b = row / (K + 1);
  const int j = (int)(row - b * (K + 1));
  const int cls = K / 2;
  T* dst = out + (size_t)row * D + c;
  float v[VEC];
  if (j == cls) {                         // (cls_token + pos_embed[:, :1]).to(x.dtype)
    float pe[VEC];
    VecIO<float, VEC>::load(cls_token + c, v);
    VecIO<float, VEC>::load(pos + c, pe);
#pragma unroll
    for (int e = 0; e < VEC; ++e) v[e] = v[e] + pe[e];
    VecIO<T, VEC>::store(dst, v);
    return;
  }
  const int r = keep[(size_t)b * K + (j - (j > cls ? 1 : 0))];
  if (r >= 0 && r < L) {
    typedef typename raw_words<VEC * sizeof(T) / 4>::type words_t;
    *reinterpret_cast<words_t*>(dst) = *reinterpret_cast<const words_t*>(x + ((size_t)b * L + r) * D + c);
    return;
  }
#pragma unroll
  for (int e = 0; e < VEC; ++e) v[e] = 0.f;
  VecIO<T, VEC>::store(dst, v);
}

// One thread per (row of dx, VEC channels).
template <typename T, int VEC>
__global__ __launch_bounds__(256) void mae_encoder_tokens_cls_bwd_kernel(const T* __restrict__ dout, const int* __restrict__ restore,
                                                                         T* __restrict__ dx, long units, int L, int K, int D) {
  const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= units) return;
  const int upr = D / VEC;
  const long row = u / upr;               // b * L + l
  const int c = (int)(u - row * upr) * VEC;
  const long b = row / L;
  const int cls = K / 2;
  const int r = restore[row];
  T* dst = dx + (size_t)row * D + c;
  if (r >= 0 && r < K) {
    typedef typename raw_words<VEC * sizeof(T) / 4>::type words_t;
    const int j = r + (r >= cls ? 1 : 0);                     // < K + 1
    *reinterpret_cast<words_t*>(dst) = *reinterpret_cast<const words_t*>(dout + ((size_t)b * (K + 1) + j) * D + c);
    return;
  }
  float v[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) v[e] = 0.f;
  VecIO<T, VEC>::store(dst, v);
}

// d cls_token: one thread per channel adds the B class rows of dout in fp64, b ascending; one rounding, to fp32.
template <typename T>
__global__ __launch_bounds__(256) void mae_cls_grad_kernel(const T* __restrict__ dout, float* __restrict__ dcls, int B, int K, int D) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= D) return;
  const size_t stride = (size_t)(K + 1) * D;
  const T* src = dout + (size_t)(K / 2) * D + d;
  double acc = 0.0;
#pragma unroll 8
  for (int b = 0; b < B; ++b) acc += (double)io<T>::ld(src + (size_t)b * stride);
  dcls[d] = (float)acc;
}

// ---- decoder input.  One thread per (output row, 4 channels).
template <typename TX>
__global__ __launch_bounds__(256) void mae_decoder_tokens_cls_fwd_kernel(const TX* __restrict__ x, const float* __restrict__ mask_token,
                                                                         const float* __restrict__ pos, const int* __restrict__ restore,
                                                                         float* __restrict__ out, long units, int L, int K, int D) {
  const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= units) return;
  const int upr = D / 4;
  const long row = u / upr;               // b * (L + 1) + l
  const int c = (int)(u - row * upr) * 4;
  const long b = row / (L + 1);
  const int l = (int)(row - b * (L + 1));
  const int cls = K / 2;
  int j = -1;                             // the row of x; -1: the mask token
  if (l == L) {
    j = cls;
  } else {
    const int r = restore[(size_t)b * L + l];
    if (r >= 0 && r < K) j = r + (r >= cls ? 1 : 0);
  }
  float v[4], pe[4];
  if (j >= 0) {
    VecIO<TX, 4>::load(x + ((size_t)b * (K + 1) + j) * D + c, v);
  } else {
    VecIO<float, 4>::load(mask_token + c, v);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = round_to_type<TX>(v[e]);      // mask_token.to(x.dtype)
  }
  VecIO<float, 4>::load(pos + (size_t)(l == L ? 0 : 1 + l) * D + c, pe);
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = v[e] + pe[e];
  VecIO<float, 4>::store(out + (size_t)row * D + c, v);
}

int cls_check(const char* who, const void* a, const void* b, const void* c, const void* d, int x_dtype, int batch, int len,
              int len_keep, int dim) {
  FV_CHECK(a && b && c && d, "%s: null pointer", who);
  FV_CHECK(batch > 0 && len > 0 && len_keep > 0 && len_keep <= len && dim > 0, "%s: empty dimension or len_keep > len", who);
  FV_CHECK(dim % 4 == 0, "%s: dim %d must be a multiple of 4", who, dim);
  FV_CHECK(f32_or_bf16(x_dtype), "%s: x must be fp32 or bf16", who);
  FV_CHECK((long)batch * ((long)len + 1) <= 0x7fffffffL, "%s: too many rows", who);
  FV_CHECK((long)batch * ((long)len + 1) * (dim / 4) <= (1L << 38), "%s: too many elements for one launch", who);
  return FV_OK;
}

}  // namespace

extern "C" int fv_mae_encoder_tokens_cls_fwd(const void* x, int x_dtype, const float* cls_token, const float* pos_embed,
                                             const int* keep_index, void* out, int batch, int len, int len_keep, int dim,
                                             fv_stream_t stream) {
  const int rc = cls_check("mae_encoder_tokens_cls_fwd", x, cls_token, pos_embed, keep_index, x_dtype, batch, len, len_keep, dim);
  if (rc != FV_OK) return rc;
  FV_CHECK(out, "mae_encoder_tokens_cls_fwd: null pointer");
  FV_CHECK(aligned_to(x, esize(x_dtype)) && aligned_to(out, esize(x_dtype)) && aligned_to(cls_token, 4) && aligned_to(pos_embed, 4) &&
               aligned_to(keep_index, 4), "mae_encoder_tokens_cls_fwd: a buffer is not aligned to its element size");
  hipStream_t st = (hipStream_t)stream;
  const bool wide = x_dtype == FV_BF16 && dim % 8 == 0;
  const long units = (long)batch * (len_keep + 1) * (dim / (wide ? 8 : 4));
  const dim3 grid(fv_cdiv(units, 256)), block(256);
#define FV_ET(T, VEC) hipLaunchKernelGGL((mae_encoder_tokens_cls_fwd_kernel<T, VEC>), grid, block, 0, st, (const T*)x, cls_token, pos_embed, keep_index, (T*)out, units, len, len_keep, dim)
  if (wide) FV_ET(bf16_t, 8);
  else if (x_dtype == FV_BF16) FV_ET(bf16_t, 4);
  else FV_ET(float, 4);
#undef FV_ET
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_mae_encoder_tokens_cls_bwd(const void* dout, const int* restore_index, void* dx, int x_dtype, float* dcls_token,
                                             int batch, int len, int len_keep, int dim, fv_stream_t stream) {
  const int rc = cls_check("mae_encoder_tokens_cls_bwd", dout, restore_index, dx, dcls_token, x_dtype, batch, len, len_keep, dim);
  if (rc != FV_OK) return rc;
  FV_CHECK(aligned_to(dout, esize(x_dtype)) && aligned_to(dx, esize(x_dtype)) && aligned_to(restore_index, 4) &&
               aligned_to(dcls_token, 4), "mae_encoder_tokens_cls_bwd: a buffer is not aligned to its element size");
  hipStream_t st = (hipStream_t)stream;
  const bool wide = x_dtype == FV_BF16 && dim % 8 == 0;
  const long units = (long)batch * len * (dim / (wide ? 8 : 4));
  const dim3 grid(fv_cdiv(units, 256)), block(256), cgrid(fv_cdiv(dim, 256));
#define FV_ET(T, VEC) hipLaunchKernelGGL((mae_encoder_tokens_cls_bwd_kernel<T, VEC>), grid, block, 0, st, (const T*)dout, restore_index, (T*)dx, units, len, len_keep, dim)
  if (wide) FV_ET(bf16_t, 8);
  else if (x_dtype == FV_BF16) FV_ET(bf16_t, 4);
  else FV_ET(float, 4);
#undef FV_ET
  if (x_dtype == FV_BF16)
    hipLaunchKernelGGL(mae_cls_grad_kernel<bf16_t>, cgrid, block, 0, st, (const bf16_t*)dout, dcls_token, batch, len_keep, dim);
  else
    hipLaunchKernelGGL(mae_cls_grad_kernel<float>, cgrid, block, 0, st, (const float*)dout, dcls_token, batch, len_keep, dim);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_mae_decoder_tokens_cls_fwd(const void* x, int x_dtype, const float* mask_token, const float* pos_embed,
                                             const int* restore_index, float* out, int batch, int len, int len_keep, int dim,
                                             fv_stream_t stream) {
  const int rc = cls_check("mae_decoder_tokens_cls_fwd", x, mask_token, pos_embed, restore_index, x_dtype, batch, len, len_keep, dim);
  if (rc != FV_OK) return rc;
  FV_CHECK(out, "mae_decoder_tokens_cls_fwd: null pointer");
  FV_CHECK(aligned_to(x, esize(x_dtype)) && aligned_to(mask_token, 4) && aligned_to(pos_embed, 4) && aligned_to(restore_index, 4) &&
               aligned_to(out, 4), "mae_decoder_tokens_cls_fwd: a buffer is not aligned to its element size");
  const long units = (long)batch * (len + 1) * (dim / 4);
  const dim3 grid(fv_cdiv(units, 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (x_dtype == FV_BF16)
    hipLaunchKernelGGL(mae_decoder_tokens_cls_fwd_kernel<bf16_t>, grid, block, 0, st, (const bf16_t*)x, mask_token, pos_embed,
                       restore_index, out, units, len, len_keep, dim);
  else
    hipLaunchKernelGGL(mae_decoder_tokens_cls_fwd_kernel<float>, grid, block, 0, st, (const float*)x, mask_token, pos_embed,
                       restore_index, out, units, len, len_keep, dim);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_mae_decoder_tokens_cls_bwd(const float* dout, const int* restore_index, void* dx, int x_dtype, double* partials,
                                             int n_partials, float* dmask_token, int batch, int len, int len_keep, int dim,
                                             fv_stream_t stream) {
  const int rc = cls_check("mae_decoder_tokens_cls_bwd", dout, restore_index, dx, partials, x_dtype, batch, len, len_keep, dim);
  if (rc != FV_OK) return rc;
  FV_CHECK(dmask_token, "mae_decoder_tokens_cls_bwd: null pointer");
  FV_CHECK(aligned_to(dout, 4) && aligned_to(restore_index, 4) && aligned_to(dx, esize(x_dtype)) && aligned_to(partials, 8) &&
               aligned_to(dmask_token, 4), "mae_decoder_tokens_cls_bwd: a buffer is not aligned to its element size");
  const long rows = (long)batch * (len + 1);
  const int nblocks = fv_cdiv(rows, DT_ROWS);
  FV_CHECK(n_partials == nblocks,
           "mae_decoder_tokens_cls_bwd: partials must hold ceil(batch (len + 1) / %d) = %d rows of dim doubles, got %d", DT_ROWS,
           nblocks, n_partials);
  const int threads = row_walk_threads(dim);
  hipStream_t st = (hipStream_t)stream;
  if (x_dtype == FV_BF16)
    hipLaunchKernelGGL((mae_decoder_tokens_bwd_kernel<bf16_t, true>), dim3(nblocks), dim3(threads), 0, st, dout, restore_index,
                       (bf16_t*)dx, partials, rows, len, len_keep, dim);
  else
    hipLaunchKernelGGL((mae_decoder_tokens_bwd_kernel<float, true>), dim3(nblocks), dim3(threads), 0, st, dout, restore_index,
                       (float*)dx, partials, rows, len, len_keep, dim);
  hipLaunchKernelGGL(mae_decoder_tokens_final_kernel, dim3(fv_cdiv(dim, 64)), dim3(64 * DT_FINAL_WAVES), 0, st,
                     (const double*)partials, dmask_token, nblocks, dim);
  FV_LAUNCH_CHECK();
  return FV_OK;
}
