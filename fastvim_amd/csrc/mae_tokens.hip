// Token bookkeeping of the MAE masked encoder (fastvim_amd/models_mae.py with ``fused_tokens``): everything that is a pure
// function of the (B, L) masking noise comes from ONE launch per step, and the permuted row copies that use it are plain
// gathers.
//   mae_mask_plan_kernel       one workgroup per sample, one thread per token.  The noise goes to LDS as order-preserving
//                              32-bit keys; rank[i] = #{j : key[j] < key[i], or equal and j < i} (a stable ascending order,
//                              L LDS broadcast reads per thread); the K lowest ranks are kept; a kept token's position among
//                              the kept ones is a ballot prefix count in token order, its position in the TRANSPOSED grid's
//                              scan order (the odd layers) the same count over the flags stored transposed.
//   mae_mask_plan_keyed_kernel the same plan of the noise of a KEY BLOCK (mask_noise.h: Philox4x32-10 of (key, step, sample, token)),
//                              generated into the LDS keys by the first L / 4 threads: the noise is never in memory.
//   mae_noise_kernel           that noise written out, (B, L) fp32: the eager form, the tests' and the fallback paths'.
//   tokens_gather_kernel       out[b, t, :] = in[b, index[b, t], :], a zero row where the index is outside [0, Lin).  A thread
//                              moves 4 (mixed / fp32) or 8 (bf16 -> bf16) channels: 16-byte accesses.  Same type in and out:
//                              a bit copy.  With unique indices the adjoint of a gather is the gather by the inverse index
//                              (-1 where a source row was not picked): one pass, no memset, no atomics, exact.
//   mae_decoder_tokens_fwd     out[b, l, :] = (r >= 0 ? x[b, r, :] : mask_token rounded to x's type) + pos[l, :], fp32 out
//                              (bf16 + fp32 promotes to fp32 in the eager chain: ONE fp32 rounding, of the sum).
//   mae_decoder_tokens_bwd     a workgroup walks DT_ROWS rows of dout: a kept row goes to dx[b, r, :] in x's type, a removed
//                              one -- rounded to x's type first, as autograd rounds it -- is added to the workgroup's fp64
//                              partial in row order; mae_decoder_tokens_final sums the partials in fp64 in a fixed order
//                              (sixteen strided walks, then a fixed tree).  No atomics: the same inputs give the same bits.
//                              Both kernels live in mae_tokens_common.h: mae_tokens_cls.hip launches them too.
// Floating-point reassociation and contraction are switched off for the whole file: every sum has ONE order, the one written.
#include "common.h"
#include "mask_noise.h"
#include "rowwalk.h"

#pragma clang fp reassociate(off) contract(off)

#include "mae_tokens_common.h"      // (behind the pragma: the fixed-order sum mae_tokens_cls.hip shares)

namespace {

constexpr int MP_MAX_L = FV_MAE_PLAN_MAX_TOKENS;

struct PlanOut {
  long long* ids_keep;      // (B, K)
  long long* ids_restore;   // (B, L)
  float* mask;              // (B, L)
  int* keep_index;          // (B, K)
  int* restore_index;       // (B, L)
  int* row_index_even;      // (2, B, K)
  long long* ids_keep_odd;  // (B, K)
  long long* order;         // (B, K)
  long long* inverse;       // (B, K)
  int* order_index;         // (B, K)
  int* inverse_index;       // (B, K)
  int* row_index_odd;       // (2, B, K)
};

// fp32 bits -> a key whose UNSIGNED order is the float order (-0 == +0).  Every bit pattern, NaN included, has a place in
// it, so the ranks are a permutation of 0 .. L-1 whatever the noise holds.
__device__ __forceinline__ uint32_t order_key(uint32_t u) {
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// exclusive prefix count of `flag` over the workgroup's threads in thread order; `totals`: one int per wave
__device__ __forceinline__ int block_prefix_count(bool flag, int* totals) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  const int before = __popcll(m & ((1ull << lane) - 1ull));
  __syncthreads();                        // (the previous use of `totals` is over)
  if (lane == 0) totals[wave] = __popcll(m);
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += totals[w];
  return base + before;
}

// The plan of one sample from its L keys in LDS (both plan kernels; the caller has synchronised behind the writes of s_key).
__device__ __forceinline__ void plan_from_keys(const uint32_t* s_key, int* s_pos, unsigned char* s_keptT, int* s_tot,
                                               const PlanOut& o, int B, int H, int W, int K) {
  const int L = H * W, b = blockIdx.x, i = threadIdx.x;       // blockDim.x >= L
  const bool live = i < L;
  int rank = 0;
  if (live) {
    const uint32_t ki = s_key[i];
    for (int j = 0; j < L; ++j) {
      const uint32_t kj = s_key[j];
      rank += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
    }
  }
  const bool kept = live && rank < K;
  const int p = block_prefix_count(kept, s_tot);              // < K: exactly K tokens have a rank below K
  if (live) {
    const bool k_ok = kept && p < K;
    const size_t bl = (size_t)b * L + i;
    o.mask[bl] = k_ok ? 0.f : 1.f;
    o.ids_restore[bl] = k_ok ? p : (rank < L ? rank : L - 1);
    o.restore_index[bl] = k_ok ? p : -1;
    s_pos[i] = k_ok ? p : -1;
    const int r = i / W, c = i - r * W;
    s_keptT[c * H + r] = k_ok ? 1 : 0;
    if (k_ok) {
      const size_t bk = (size_t)b * K;
      o.ids_keep[bk + p] = i;
      o.keep_index[bk + p] = i;
      o.row_index_even[bk + p] = r;
      o.row_index_even[(size_t)B * K + bk + (K - 1 - p)] = (H - 1) - r;
    }
  }
  __syncthreads();
  // thread t now stands for place t of the transposed grid (W rows of H): token (t % H) * W + t / H
  const bool keptT = live && s_keptT[i] != 0;
  const int q = block_prefix_count(keptT, s_tot);
  if (keptT && q < K) {
    const int rt = i / H, ct = i - rt * H;
    const int pp = s_pos[ct * W + rt];                        // in [0, K): the flag was set by that token
    const size_t bk = (size_t)b * K;
    o.ids_keep_odd[bk + q] = i;
    o.order[bk + q] = pp;
    o.order_index[bk + q] = pp;
    o.inverse[bk + pp] = q;
    o.inverse_index[bk + pp] = q;
    o.row_index_odd[bk + q] = rt;
    o.row_index_odd[(size_t)B * K + bk + (K - 1 - q)] = (W - 1) - rt;
  }
}

__global__ __launch_bounds__(1024) void mae_mask_plan_kernel(const float* __restrict__ noise, PlanOut o, int B, int H, int W,
                                                             int K) {
  __shared__ uint32_t s_key[MP_MAX_L];
  __shared__ int s_pos[MP_MAX_L];             // kept position of token i, -1 = removed
  __shared__ unsigned char s_keptT[MP_MAX_L]; // kept flag at the token's place in the transposed grid
  __shared__ int s_tot[16];
  const int L = H * W, b = blockIdx.x, i = threadIdx.x;       // blockDim.x >= L
  if (i < L) s_key[i] = order_key(__float_as_uint(noise[(size_t)b * L + i]));
  __syncthreads();
  plan_from_keys(s_key, s_pos, s_keptT, s_tot, o, B, H, W, K);
}

// The same plan with the noise made here (mask_noise.h) instead of loaded: thread t < ceil(L / 4) runs the Philox rounds of
// token group t and puts its (up to) four keys into LDS; no (B, L) tensor exists.
__global__ __launch_bounds__(1024) void mae_mask_plan_keyed_kernel(const int32_t* __restrict__ block, PlanOut o, int B, int H,
                                                                   int W, int K) {
  __shared__ uint32_t s_key[MP_MAX_L];
  __shared__ int s_pos[MP_MAX_L];
  __shared__ unsigned char s_keptT[MP_MAX_L];
  __shared__ int s_tot[16];
  const int L = H * W, b = blockIdx.x, t = threadIdx.x;       // blockDim.x >= L >= ceil(L / 4)
  if (4 * t < L) {
    float u[4];
    fv_mask::noise4(fv_mask::load_key(block), b, t, u);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (4 * t + k < L) s_key[4 * t + k] = order_key(__float_as_uint(u[k]));
  }
  __syncthreads();
  plan_from_keys(s_key, s_pos, s_keptT, s_tot, o, B, H, W, K);
}

// noise (B, L) fp32 of the key block: one thread per (sample, group of four tokens)
__global__ __launch_bounds__(256) void mae_noise_kernel(const int32_t* __restrict__ block, float* __restrict__ noise, long units,
                                                        int G, int L) {
  const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= units) return;
  const long b = v / G;
  const int g = (int)(v - b * G);
  float u[4];
  fv_mask::noise4(fv_mask::load_key(block), (int)b, g, u);
  float* dst = noise + (size_t)b * L + 4 * g;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (4 * g + k < L) dst[k] = u[k];
}

// ---- row gather.  One thread per (output row, VEC channels).
template <typename TI, typename TO, int VEC>
__global__ __launch_bounds__(256) void tokens_gather_kernel(const TI* __restrict__ in, const int* __restrict__ index,
                                                            TO* __restrict__ out, long units, int Lin, int Lout, int D) {
  const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= units) return;
  const int upr = D / VEC;                // units per row
  const long row = u / upr;               // b * Lout + t
  const int c = (int)(u - row * upr) * VEC;
  const long b = row / Lout;
  const int r = index[row];
  float v[VEC];
  if (r >= 0 && r < Lin) {
    const TI* src = in + ((size_t)b * Lin + r) * D + c;
    if constexpr (sizeof(TI) == sizeof(TO)) {                 // the same type: the bits, untouched
      typedef typename raw_words<VEC * sizeof(TI) / 4>::type words_t;
      *reinterpret_cast<words_t*>(out + (size_t)row * D + c) = *reinterpret_cast<const words_t*>(src);
      return;
    } else {
      VecIO<TI, VEC>::load(src, v);
    }
  } else {
#pragma unroll
    for (int e = 0; e < VEC; ++e) v[e] = 0.f;
  }
  VecIO<TO, VEC>::store(out + (size_t)row * D + c, v);
}

// ---- decoder input.  One thread per (row, 4 channels).
template <typename TX>
__global__ __launch_bounds__(256) void mae_decoder_tokens_fwd_kernel(const TX* __restrict__ x, const float* __restrict__ mask_token,
                                                                     const float* __restrict__ pos, const int* __restrict__ restore,
                                                                     float* __restrict__ out, long units, int L, int K, int D) {
  const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= units) return;
  const int upr = D / 4;
  const long row = u / upr;               // b * L + l
  const int c = (int)(u - row * upr) * 4;
  const long b = row / L;
  const int l = (int)(row - b * L);
  const int r = restore[row];
  float v[4], pe[4];
  if (r >= 0 && r < K) {
    VecIO<TX, 4>::load(x + ((size_t)b * K + r) * D + c, v);
  } else {
    VecIO<float, 4>::load(mask_token + c, v);
    if constexpr (sizeof(TX) == 2) {      // mask_token.to(x.dtype): round to nearest even, then widen again
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = bf16_bits_to_f32(f32_to_bf16_bits(v[e]));
    }
  }
  VecIO<float, 4>::load(pos + (size_t)l * D + c, pe);
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = v[e] + pe[e];
  VecIO<float, 4>::store(out + (size_t)row * D + c, v);
}

}  // namespace

namespace {
// the checks both plan entry points share; `src` is the noise tensor or the key block (4-byte elements either way)
int plan_check(const char* who, const void* src, const PlanOut& o, int batch, int grid_h, int grid_w, int len_keep) {
  FV_CHECK(src && o.ids_keep && o.ids_restore && o.mask && o.keep_index && o.restore_index && o.row_index_even && o.ids_keep_odd &&
               o.order && o.inverse && o.order_index && o.inverse_index && o.row_index_odd, "%s: null pointer", who);
  FV_CHECK(batch > 0 && grid_h > 0 && grid_w > 0 && (long)grid_h * grid_w <= MP_MAX_L,
           "%s: batch %d, grid %d x %d: needs a non-empty grid of at most %d tokens", who, batch, grid_h, grid_w, MP_MAX_L);
  FV_CHECK(len_keep >= 1 && len_keep <= grid_h * grid_w, "%s: len_keep %d outside [1, %d]", who, len_keep, grid_h * grid_w);
  FV_CHECK(aligned_to(src, 4) && aligned_to(o.mask, 4) && aligned_to(o.keep_index, 4) && aligned_to(o.restore_index, 4) &&
               aligned_to(o.row_index_even, 4) && aligned_to(o.order_index, 4) && aligned_to(o.inverse_index, 4) &&
               aligned_to(o.row_index_odd, 4) && aligned_to(o.ids_keep, 8) && aligned_to(o.ids_restore, 8) &&
               aligned_to(o.ids_keep_odd, 8) && aligned_to(o.order, 8) && aligned_to(o.inverse, 8),
           "%s: a buffer is not aligned to its element size", who);
  return FV_OK;
}
int plan_threads(int L) { return ((L + FV_WAVE - 1) / FV_WAVE) * FV_WAVE; }        // one thread per token, whole waves
}  // namespace

extern "C" int fv_mae_mask_plan(const float* noise, long long* ids_keep, long long* ids_restore, float* mask, int* keep_index,
                                int* restore_index, int* row_index_even, long long* ids_keep_odd, long long* order,
                                long long* inverse, int* order_index, int* inverse_index, int* row_index_odd, int batch,
                                int grid_h, int grid_w, int len_keep, fv_stream_t stream) {
  PlanOut o{ids_keep, ids_restore, mask, keep_index, restore_index, row_index_even, ids_keep_odd, order, inverse, order_index,
            inverse_index, row_index_odd};
  const int rc = plan_check("mae_mask_plan", noise, o, batch, grid_h, grid_w, len_keep);
  if (rc != FV_OK) return rc;
  hipLaunchKernelGGL(mae_mask_plan_kernel, dim3(batch), dim3(plan_threads(grid_h * grid_w)), 0, (hipStream_t)stream, noise, o,
                     batch, grid_h, grid_w, len_keep);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_mae_noise(const int32_t* block, float* noise, int batch, int len, fv_stream_t stream) {
  FV_CHECK(block && noise, "mae_noise: null pointer");
  FV_CHECK(batch > 0 && len > 0, "mae_noise: batch %d, len %d: empty", batch, len);
  FV_CHECK(aligned_to(block, 4) && aligned_to(noise, 4), "mae_noise: a buffer is not aligned to its element size");
  const int G = (len + 3) / 4;
  const long units = (long)batch * G;
  FV_CHECK(units <= 0x7fffffffL, "mae_noise: too many tokens");
  hipLaunchKernelGGL(mae_noise_kernel, dim3(fv_cdiv(units, 256)), dim3(256), 0, (hipStream_t)stream, block, noise, units, G, len);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_mae_mask_plan_keyed(const int32_t* block, long long* ids_keep, long long* ids_restore, float* mask,
                                      int* keep_index, int* restore_index, int* row_index_even, long long* ids_keep_odd,
                                      long long* order, long long* inverse, int* order_index, int* inverse_index,
                                      int* row_index_odd, int batch, int grid_h, int grid_w, int len_keep, fv_stream_t stream) {
  PlanOut o{ids_keep, ids_restore, mask, keep_index, restore_index, row_index_even, ids_keep_odd, order, inverse, order_index,
            inverse_index, row_index_odd};
  const int rc = plan_check("mae_mask_plan_keyed", block, o, batch, grid_h, grid_w, len_keep);
  if (rc != FV_OK) return rc;
  hipLaunchKernelGGL(mae_mask_plan_keyed_kernel, dim3(batch), dim3(plan_threads(grid_h * grid_w)), 0, (hipStream_t)stream, block,
                     o, batch, grid_h, grid_w, len_keep);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_tokens_gather(const void* in, int in_dtype, const int* index, void* out, int out_dtype, int batch, int len_in,
                                int len_out, int dim, fv_stream_t stream) {
  FV_CHECK(in && index && out, "tokens_gather: null pointer");
  FV_CHECK(batch > 0 && len_in > 0 && len_out > 0 && dim > 0, "tokens_gather: empty dimension");
  FV_CHECK(dim % 4 == 0, "tokens_gather: dim %d must be a multiple of 4", dim);
  FV_CHECK(f32_or_bf16(in_dtype) && f32_or_bf16(out_dtype), "tokens_gather: dtypes must be fp32 or bf16");
  FV_CHECK(aligned_to(in, esize(in_dtype)) && aligned_to(out, esize(out_dtype)) && aligned_to(index, 4),
           "tokens_gather: a buffer is not aligned to its element size");
  FV_CHECK((long)batch * len_in <= 0x7fffffffL && (long)batch * len_out <= 0x7fffffffL, "tokens_gather: too many rows");
  hipStream_t st = (hipStream_t)stream;
  const bool wide = in_dtype == FV_BF16 && out_dtype == FV_BF16 && dim % 8 == 0;
  const long units = (long)batch * len_out * (dim / (wide ? 8 : 4));
  const dim3 grid(fv_cdiv(units, 256)), block(256);
#define FV_TG(TI, TO, VEC) hipLaunchKernelGGL((tokens_gather_kernel<TI, TO, VEC>), grid, block, 0, st, (const TI*)in, index, (TO*)out, units, len_in, len_out, dim)
  if (wide) FV_TG(bf16_t, bf16_t, 8);
  else if (in_dtype == FV_BF16 && out_dtype == FV_BF16) FV_TG(bf16_t, bf16_t, 4);
  else if (in_dtype == FV_BF16) FV_TG(bf16_t, float, 4);
  else if (out_dtype == FV_BF16) FV_TG(float, bf16_t, 4);
  else FV_TG(float, float, 4);
#undef FV_TG
  FV_LAUNCH_CHECK();
  return FV_OK;
}

namespace {
int decoder_check(const char* who, const void* a, const void* b, const void* c, const void* d, int x_dtype, int batch, int len,
                  int len_keep, int dim) {
  FV_CHECK(a && b && c && d, "%s: null pointer", who);
  FV_CHECK(batch > 0 && len > 0 && len_keep > 0 && len_keep <= len && dim > 0, "%s: empty dimension or len_keep > len", who);
  FV_CHECK(dim % 4 == 0, "%s: dim %d must be a multiple of 4", who, dim);
  FV_CHECK(f32_or_bf16(x_dtype), "%s: x must be fp32 or bf16", who);
  FV_CHECK((long)batch * len <= 0x7fffffffL, "%s: too many rows", who);
  return FV_OK;
}
}  // namespace

extern "C" int fv_mae_decoder_tokens_fwd(const void* x, int x_dtype, const float* mask_token, const float* pos_embed,
                                         const int* restore_index, float* out, int batch, int len, int len_keep, int dim,
                                         fv_stream_t stream) {
  const int rc = decoder_check("mae_decoder_tokens_fwd", x, mask_token, pos_embed, restore_index, x_dtype, batch, len, len_keep, dim);
  if (rc != FV_OK) return rc;
  FV_CHECK(out, "mae_decoder_tokens_fwd: null pointer");
  FV_CHECK(aligned_to(x, esize(x_dtype)) && aligned_to(mask_token, 4) && aligned_to(pos_embed, 4) && aligned_to(restore_index, 4) &&
               aligned_to(out, 4), "mae_decoder_tokens_fwd: a buffer is not aligned to its element size");
  const long units = (long)batch * len * (dim / 4);
  const dim3 grid(fv_cdiv(units, 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (x_dtype == FV_BF16)
    hipLaunchKernelGGL(mae_decoder_tokens_fwd_kernel<bf16_t>, grid, block, 0, st, (const bf16_t*)x, mask_token, pos_embed,
                       restore_index, out, units, len, len_keep, dim);
  else
    hipLaunchKernelGGL(mae_decoder_tokens_fwd_kernel<float>, grid, block, 0, st, (const float*)x, mask_token, pos_embed,
                       restore_index, out, units, len, len_keep, dim);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_mae_decoder_tokens_bwd(const float* dout, const int* restore_index, void* dx, int x_dtype, double* partials,
                                         int n_partials, float* dmask_token, int batch, int len, int len_keep, int dim,
                                         fv_stream_t stream) {
  const int rc = decoder_check("mae_decoder_tokens_bwd", dout, restore_index, dx, partials, x_dtype, batch, len, len_keep, dim);
  if (rc != FV_OK) return rc;
  FV_CHECK(dmask_token, "mae_decoder_tokens_bwd: null pointer");
  FV_CHECK(aligned_to(dout, 4) && aligned_to(restore_index, 4) && aligned_to(dx, esize(x_dtype)) && aligned_to(partials, 8) &&
               aligned_to(dmask_token, 4), "mae_decoder_tokens_bwd: a buffer is not aligned to its element size");
  const long rows = (long)batch * len;
  const int nblocks = fv_cdiv(rows, DT_ROWS);
  FV_CHECK(n_partials == nblocks, "mae_decoder_tokens_bwd: partials must hold ceil(batch len / %d) = %d rows of dim doubles, got %d",
           DT_ROWS, nblocks, n_partials);
  const int threads = row_walk_threads(dim);
  hipStream_t st = (hipStream_t)stream;
  if (x_dtype == FV_BF16)
    hipLaunchKernelGGL((mae_decoder_tokens_bwd_kernel<bf16_t, false>), dim3(nblocks), dim3(threads), 0, st, dout, restore_index, (bf16_t*)dx,
                       partials, rows, len, len_keep, dim);
  else
    hipLaunchKernelGGL((mae_decoder_tokens_bwd_kernel<float, false>), dim3(nblocks), dim3(threads), 0, st, dout, restore_index, (float*)dx,
                       partials, rows, len, len_keep, dim);
  hipLaunchKernelGGL(mae_decoder_tokens_final_kernel, dim3(fv_cdiv(dim, 64)), dim3(64 * DT_FINAL_WAVES), 0, st,
                     (const double*)partials, dmask_token, nblocks, dim);
  FV_LAUNCH_CHECK();
  return FV_OK;
}
