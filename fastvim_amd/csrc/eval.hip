// The validation step's two launch families.
// Replaces, per validation batch of the reference (imagenet_classification/supervised_imagenet.py:151-210,
// mae/finetune_imagenet.py:165-221, cell_imaging/supervised.py:132-165: the live backbone and self.ema.module on the same
// batch, F.cross_entropy + torchmetrics Accuracy for each, logged as epoch means):
//   swap_params_ema_kernel   param <-> ema, element for element, and shadow = cast(new param) in ONE pass: the model's
//                            forward reads the EMA weights through the very buffers it reads the live weights through,
//                            and a second swap puts everything back bit for bit.  8 B read + 8 B + sizeof(shadow)
//                            written per element (18 B with a bf16 shadow); no arithmetic on the values.
//   eval_rows_kernel         cross-entropy and top-1 flag of the rows b < *n_valid: the row body of fv_label_ce
//                            (csrc/ce_row.h), smoothing 0 -- the same bits in loss_rows / correct_rows
//   eval_accumulate_kernel   ONE workgroup adds the batch into the device accumulator block: the fp64 sum of the fp32 row
//                            losses in a fixed order (no float atomics), the row and correct counts, and the per-class
//                            label / correct counts (integer atomics)
// n_valid is read from device memory when the kernels RUN: a captured launch serves the short last batch of an epoch.
#include "common.h"
#include "ce_row.h"

namespace {

using namespace fv_ce_row;

// ------------------------------------------------------------------------------------------------ swap
// the shadow's dtype: one element, and four consecutive ones as one store (the destination aligned to 4 elements)
__device__ __forceinline__ void shadow_st1(bf16_t* s, float v) {
  *reinterpret_cast<uint16_t*>(s) = f32_to_bf16_bits(v);                   // round to nearest even, a NaN stays a NaN
}
__device__ __forceinline__ void shadow_st1(__half* s, float v) { *s = __float2half_rn(v); }
__device__ __forceinline__ void shadow_st1(float* s, float v) { *s = v; }
__device__ __forceinline__ void shadow_st4(bf16_t* s, float4 v) {
  const uint2 pk = {pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w)};         // (the optimizer kernels' cast)
  *reinterpret_cast<uint2*>(s) = pk;
}
__device__ __forceinline__ void shadow_st4(__half* s, float4 v) {
  const __half2 lo = __floats2half2_rn(v.x, v.y), hi = __floats2half2_rn(v.z, v.w);
  const uint2 pk = {*reinterpret_cast<const uint32_t*>(&lo), *reinterpret_cast<const uint32_t*>(&hi)};
  *reinterpret_cast<uint2*>(s) = pk;
}
__device__ __forceinline__ void shadow_st4(float* s, float4 v) { *reinterpret_cast<float4*>(s) = v; }

// Elements [head, head + 4 n4) as 16-byte accesses (the launcher picks `head` so that all three buffers are aligned
// there, or n4 = 0 when no such head exists); the `head` elements before and the < 4 after them one at a time.
template <typename S>
__global__ __launch_bounds__(256) void swap_params_ema_kernel(float* p, float* e, S* s, size_t n, size_t head, size_t n4) {
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  float4* p4 = reinterpret_cast<float4*>(p + head);
  float4* e4 = reinterpret_cast<float4*>(e + head);
  S* sb = s + head;
  for (size_t i = gid; i < n4; i += stride) {
    const float4 a = p4[i], b = e4[i];
    p4[i] = b;
    e4[i] = a;
    shadow_st4(sb + 4 * i, b);
  }
  const size_t tail0 = head + 4 * n4;
  const size_t n_edge = head + (n - tail0);
  for (size_t j = gid; j < n_edge; j += stride) {
    const size_t i = j < head ? j : tail0 + (j - head);
    const float a = p[i], b = e[i];
    p[i] = b;
    e[i] = a;
    shadow_st1(s + i, b);
  }
}

template <typename S>
void launch_swap(float* p, float* e, void* shadow, size_t n, hipStream_t st) {
  // elements up to the next 16-byte boundary of param; the wide body needs ema and the shadow aligned at the same element
  size_t head = (4 - (((uintptr_t)p >> 2) & 3)) & 3;
  if (head > n) head = n;
  size_t n4 = (n - head) / 4;
  const bool wide = (((uintptr_t)(p + head) | (uintptr_t)(e + head)) & 15) == 0 &&
                    ((uintptr_t)((S*)shadow + head) & (4 * sizeof(S) - 1)) == 0;
  if (!wide) { head = 0; n4 = 0; }
  const size_t n_edge = n - 4 * n4;
  const size_t work = n4 > n_edge ? n4 : n_edge;
  size_t blocks = (work + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(swap_params_ema_kernel<S>, dim3((unsigned)blocks), dim3(256), 0, st, p, e, (S*)shadow, n, head, n4);
}

// ------------------------------------------------------------------------------------------------ metrics
// label_ce_rows_kernel<T, false> of csrc/loss.hip with the row count read from the device.  The arguments the row body
// sees are run-time values there and here (on / off; dx, which the launcher passes as null), so the compiler is given the
// same body to compile.  A row at or past *n_valid is not read; its scratch entries are zeroed.
template <typename T>
__global__ __launch_bounds__(256) void eval_rows_kernel(const T* __restrict__ x, const int64_t* __restrict__ labels,
                                                         const int32_t* __restrict__ n_valid, float on, float off,
                                                         float* __restrict__ loss_rows, float* __restrict__ dx,
                                                         int32_t* __restrict__ correct_rows, int B, int C, float inv_b) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= B) return;
  if (row >= n_valid[0]) {
    if ((threadIdx.x & 63) == 0) {
      loss_rows[row] = 0.f;
      correct_rows[row] = 0;
    }
    return;
  }
  LabelTarget<false> ts;
  ts.label = labels[row];          // compared with class indices only, never used as an index: any value is safe
  ts.partner = -1;
  ts.on = on; ts.off = off;
  ts.lam = 1.f; ts.oml = 0.f;
  soft_ce_row_body<T>(x + (size_t)row * C, ts, loss_rows, dx, correct_rows, row, C, inv_b);
}

// One workgroup of 256.  Thread t sums rows t, t + 256, ... in fp64, then the butterfly over the wave, then the four
// waves in order: one fixed association per (batch, n_valid).  Only thread 0 touches the three scalars, and launches on a
// stream run one after the other, so the block's bytes depend on the batches and their order alone.
__global__ __launch_bounds__(256) void eval_accumulate_kernel(const float* __restrict__ loss_rows,
                                                              const int32_t* __restrict__ correct_rows,
                                                              const int64_t* __restrict__ labels,
                                                              const int32_t* __restrict__ n_valid, int64_t* acc, int B, int C) {
#pragma clang fp reassociate(off) contract(off)
  __shared__ double s_sum[4];
  __shared__ int s_cnt[4];
  const int tid = threadIdx.x;
  int nv = n_valid[0];
  nv = nv < 0 ? 0 : (nv > B ? B : nv);
  unsigned long long* support = reinterpret_cast<unsigned long long*>(acc) + FV_EVAL_ACC_HEAD;
  unsigned long long* hit = support + C;
  double s = 0.0;
  int nc = 0;
  for (int b = tid; b < nv; b += 256) {
    s += (double)loss_rows[b];
    const int ok = correct_rows[b];
    nc += ok;
    const int64_t lab = labels[b];
    if (lab >= 0 && lab < (int64_t)C) {            // a label outside [0, classes) is seen, and counted in no class
      atomicAdd(support + lab, 1ull);
      if (ok) atomicAdd(hit + lab, 1ull);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o);
    nc += __shfl_xor(nc, o);
  }
  if ((tid & 63) == 0) {
    s_sum[tid >> 6] = s;
    s_cnt[tid >> 6] = nc;
  }
  __syncthreads();
  if (tid == 0) {
    const double batch_sum = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
    double* loss_sum = reinterpret_cast<double*>(acc);
    loss_sum[0] = loss_sum[0] + batch_sum;
    acc[1] += (int64_t)nv;
    acc[2] += (int64_t)(s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]);
  }
}

}  // namespace

extern "C" int fv_swap_params_ema(float* params, float* ema, void* shadow, int shadow_dtype, size_t n, fv_stream_t stream) {
  FV_CHECK(params && ema && shadow, "swap_params_ema: null pointer");
  FV_CHECK(shadow_dtype == FV_F32 || shadow_dtype == FV_BF16 || shadow_dtype == FV_F16,
           "swap_params_ema: the shadow must be fp32, bf16 or fp16 (got dtype code %d)", shadow_dtype);
  FV_CHECK((((uintptr_t)params | (uintptr_t)ema) & 3) == 0 &&
               ((uintptr_t)shadow & (shadow_dtype == FV_F32 ? 3 : 1)) == 0,
           "swap_params_ema: a buffer is not aligned to its element size");
  FV_CHECK(params != ema, "swap_params_ema: params and ema are the same buffer");
  if (n == 0) return FV_OK;
  hipStream_t st = (hipStream_t)stream;
  if (shadow_dtype == FV_BF16) launch_swap<bf16_t>(params, ema, shadow, n, st);
  else if (shadow_dtype == FV_F16) launch_swap<__half>(params, ema, shadow, n, st);
  else launch_swap<float>(params, ema, shadow, n, st);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_eval_accumulate(const void* logits, int logits_dtype, const int64_t* labels, const int32_t* n_valid,
                                  float* loss_rows, int32_t* correct_rows, int64_t* acc, int batch, int classes,
                                  fv_stream_t stream) {
  FV_CHECK(logits && labels && n_valid && loss_rows && correct_rows && acc, "eval_accumulate: null pointer");
  FV_CHECK(batch > 0 && classes > 0, "eval_accumulate: empty dimension");
  FV_CHECK(classes <= 64 * EPL, "eval_accumulate: at most %d classes (got %d)", 64 * EPL, classes);
  FV_CHECK(logits_dtype == FV_F32 || logits_dtype == FV_BF16, "eval_accumulate: logits must be fp32 or bf16");
  FV_CHECK(((uintptr_t)acc & 7) == 0, "eval_accumulate: the accumulator block must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const float inv_b = 1.f / (float)batch;
  const dim3 grid(fv_cdiv(batch, 4)), block(256);
  // smoothing 0 of fv_label_ce: on = 1, off = 0
  if (logits_dtype == FV_F32)
    hipLaunchKernelGGL(eval_rows_kernel<float>, grid, block, 0, st, (const float*)logits, labels, n_valid, 1.f, 0.f, loss_rows,
                       (float*)nullptr, correct_rows, batch, classes, inv_b);
  else
    hipLaunchKernelGGL(eval_rows_kernel<bf16_t>, grid, block, 0, st, (const bf16_t*)logits, labels, n_valid, 1.f, 0.f,
                       loss_rows, (float*)nullptr, correct_rows, batch, classes, inv_b);
  hipLaunchKernelGGL(eval_accumulate_kernel, dim3(1), dim3(256), 0, st, (const float*)loss_rows, (const int32_t*)correct_rows,
                     labels, n_valid, acc, batch, classes);
  FV_LAUNCH_CHECK();
  return FV_OK;
}
