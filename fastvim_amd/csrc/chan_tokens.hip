// Class-token assembly of the ChannelVim baseline (fastvim_amd/models_channel_mamba.py with ``fused_cls``): the M = P C'
// channel tokens of a sample -- ``pos_embed`` is already in them, added by the channel patch projection's epilogue -- with
// the class token put in at place p (M / 2, "the middle channel's middle token").  Nothing is added on the way: unlike
// vim_tokens.hip there is no position table here, so the token rows are MOVED (a -0.0 stays -0.0, a NaN keeps its payload)
// and the backward has no sum over the batch but the class row's.
//   chan_cls_tokens_fwd  out (B, M + 1, D) in T from y (B, M, D) in T (fp32 or bf16): row j is cls_token rounded to T when
//                        j == p, else the bits of y[b, j - (j > p)].  A thread moves 16 bytes (bf16 with D % 8 != 0: 8).
//   chan_cls_tokens_bwd  from dout (B, M + 1, D) in T: dy[b, i] = the bits of dout[b, i + (i >= p)], one thread per 16 bytes
//                        over the whole of dy; d cls_token[d] the sum over b = 0 .. B-1 of dout[b, p, d], in fp64 in that
//                        order, rounded once to fp32 -- D / VEC threads of the SAME launch that walk the batch.  Their
//                        workgroups are the first of the grid: they are dispatched first and walk under the copy.
// No atomics, no partial buffer, nothing that waits for the host.  Floating-point reassociation and contraction are switched
// off for the whole file: the one sum has ONE order, the one written.
#include "common.h"
#include "rowwalk.h"

#pragma clang fp reassociate(off) contract(off)

#include "mae_tokens_common.h"      // the argument checks (behind the pragma)

namespace {

constexpr int CT_THREADS = 256;

// VEC elements of T as raw 32-bit words: what a row copy moves
template <typename T, int VEC>
__device__ __forceinline__ void move_bits(const T* __restrict__ src, T* __restrict__ dst) {
  constexpr int W = VEC * (int)sizeof(T) / 4;
  typedef typename raw_words<W>::type words_t;
  *reinterpret_cast<words_t*>(dst) = *reinterpret_cast<const words_t*>(src);
}

// unit u of a (rows of len1 per sample, upr units per row) tensor -> (sample, row of the sample, first channel).  32-bit
// divisions wherever the unit count allows them (a 64-bit one costs more than the 16 bytes it places).
template <int VEC>
__device__ __forceinline__ void place(long u, bool small, int upr, int len1, long& b, int& j, int& c) {
  if (small) {
    const unsigned uu = (unsigned)u;
    const unsigned row = uu / (unsigned)upr;
    c = (int)(uu - row * (unsigned)upr) * VEC;
    const unsigned bb = row / (unsigned)len1;
    b = bb;
    j = (int)(row - bb * (unsigned)len1);
  } else {
    const long row = u / upr;
    c = (int)(u - row * upr) * VEC;
    b = row / len1;
    j = (int)(row - b * len1);
  }
}

template <typename T, int VEC>
__global__ __launch_bounds__(CT_THREADS) void chan_cls_tokens_fwd_kernel(const T* __restrict__ y, const float* __restrict__ cls_token,
                                                                         T* __restrict__ out, long units, int small, int M,
                                                                         int D, int p) {
  const long u = (long)blockIdx.x * CT_THREADS + threadIdx.x;
  if (u >= units) return;
  long b;
  int j, c;
  place<VEC>(u, small != 0, D / VEC, M + 1, b, j, c);
  T* dst = out + ((size_t)b * (M + 1) + j) * D + c;
  if (j == p) {                           // cls_token.expand(B, -1, -1).to(x.dtype)
    float v[VEC];
    VecIO<float, VEC>::load(cls_token + c, v);
    VecIO<T, VEC>::store(dst, v);
  } else {
    move_bits<T, VEC>(y + ((size_t)b * M + (j - (j > p ? 1 : 0))) * D + c, dst);
  }
}

// Workgroups [0, sum_blocks): thread t < D / VEC owns VEC channels of the class row and walks the batch in order, UNR
// samples' loads in flight.  Workgroups behind them: one thread per VEC channels of dy.
template <typename T, int VEC>
__global__ __launch_bounds__(CT_THREADS) void chan_cls_tokens_bwd_kernel(const T* __restrict__ dout, T* __restrict__ dy,
                                                                         float* __restrict__ dcls, long units, int small,
                                                                         int sum_blocks, int B, int M, int D, int p) {
  if ((int)blockIdx.x < sum_blocks) {
    constexpr int UNR = 32 / VEC;         // (32 values in flight: the copy threads of the same kernel keep their occupancy)
    const int c = ((int)blockIdx.x * CT_THREADS + (int)threadIdx.x) * VEC;
    if (c >= D) return;
    const size_t stride = (size_t)(M + 1) * D;
    const T* src = dout + (size_t)p * D + c;
    double acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.0;
    int b = 0;
    for (; b + UNR <= B; b += UNR) {
      float v[UNR][VEC];
#pragma unroll
      for (int k = 0; k < UNR; ++k) VecIO<T, VEC>::load(src + (size_t)(b + k) * stride, v[k]);
#pragma unroll
      for (int k = 0; k < UNR; ++k) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] += (double)v[k][e];
      }
    }
    for (; b < B; ++b) {
      float v[VEC];
      VecIO<T, VEC>::load(src + (size_t)b * stride, v);
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[e] += (double)v[e];
    }
    float o[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) o[e] = (float)acc[e];
    VecIO<float, VEC>::store(dcls + c, o);
    return;
  }
  const long u = (long)((int)blockIdx.x - sum_blocks) * CT_THREADS + threadIdx.x;
  if (u >= units) return;
  long b;
  int i, c;
  place<VEC>(u, small != 0, D / VEC, M, b, i, c);
  move_bits<T, VEC>(dout + ((size_t)b * (M + 1) + (i + (i >= p ? 1 : 0))) * D + c, dy + ((size_t)b * M + i) * D + c);
}

int chan_check(const char* who, const void* a, const void* b, const void* c, int dtype, int batch, int len, int dim,
               int position) {
  FV_CHECK(a && b && c, "%s: null pointer", who);
  FV_CHECK(batch > 0 && len > 0 && dim > 0, "%s: empty dimension", who);
  FV_CHECK(position >= 0 && position <= len, "%s: the class position %d is not in 0 .. %d", who, position, len);
  FV_CHECK(dim % 4 == 0, "%s: dim %d must be a multiple of 4", who, dim);
  FV_CHECK(f32_or_bf16(dtype), "%s: the tokens must be fp32 or bf16", who);
  FV_CHECK((long)batch * ((long)len + 1) <= 0x7fffffffL, "%s: too many rows", who);
  FV_CHECK((long)batch * ((long)len + 1) * (dim / 4) <= (1L << 38), "%s: too many elements for one launch", who);
  return FV_OK;
}

}  // namespace

extern "C" int fv_chan_cls_tokens_fwd(const void* y, int dtype, const float* cls_token, void* out, int batch, int len, int dim,
                                      int position, fv_stream_t stream) {
  const int rc = chan_check("chan_cls_tokens_fwd", y, cls_token, out, dtype, batch, len, dim, position);
  if (rc != FV_OK) return rc;
  FV_CHECK(aligned_to(y, 4) && aligned_to(cls_token, 4) && aligned_to(out, 4), "chan_cls_tokens_fwd: a buffer is not 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const bool wide = dtype == FV_BF16 && dim % 8 == 0;
  const long units = (long)batch * (len + 1) * (dim / (wide ? 8 : 4));
  const int small = units <= 0xffffffffL ? 1 : 0;
  const dim3 grid(fv_cdiv(units, CT_THREADS)), block(CT_THREADS);
#define FV_CT(T, VEC) hipLaunchKernelGGL((chan_cls_tokens_fwd_kernel<T, VEC>), grid, block, 0, st, (const T*)y, cls_token, (T*)out, units, small, len, dim, position)
  if (wide) FV_CT(bf16_t, 8);
  else if (dtype == FV_BF16) FV_CT(bf16_t, 4);
  else FV_CT(float, 4);
#undef FV_CT
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_chan_cls_tokens_bwd(const void* dout, void* dy, int dtype, float* dcls_token, int batch, int len, int dim,
                                      int position, fv_stream_t stream) {
  const int rc = chan_check("chan_cls_tokens_bwd", dout, dy, dcls_token, dtype, batch, len, dim, position);
  if (rc != FV_OK) return rc;
  FV_CHECK(aligned_to(dout, 4) && aligned_to(dy, 4) && aligned_to(dcls_token, 4), "chan_cls_tokens_bwd: a buffer is not 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const bool wide = dtype == FV_BF16 && dim % 8 == 0;
  const int vec = wide ? 8 : 4;
  const long units = (long)batch * len * (dim / vec);
  const int small = units <= 0xffffffffL ? 1 : 0;
  const int sum_blocks = fv_cdiv(dim / vec, CT_THREADS);
  const dim3 grid(sum_blocks + fv_cdiv(units, CT_THREADS)), block(CT_THREADS);
#define FV_CT(T, VEC) hipLaunchKernelGGL((chan_cls_tokens_bwd_kernel<T, VEC>), grid, block, 0, st, (const T*)dout, (T*)dy, dcls_token, units, small, sum_blocks, batch, len, dim, position)
  if (wide) FV_CT(bf16_t, 8);
  else if (dtype == FV_BF16) FV_CT(bf16_t, 4);
  else FV_CT(float, 4);
#undef FV_CT
  FV_LAUNCH_CHECK();
  return FV_OK;
}
