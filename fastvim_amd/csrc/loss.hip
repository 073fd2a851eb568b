// Soft-target cross-entropy, forward and gradient in one launch.
// Replaces, per training step of the reference (imagenet_classification/supervised_imagenet.py:83, 109-115:
// timm.loss.SoftTargetCrossEntropy under mixup / label smoothing): logits.float(), log_softmax, mul, neg, sum, mean
// and their five autograd kernels --
//     loss_b = sum_c -t[b][c] * log_softmax(x[b])[c],      loss = mean_b loss_b
//     d loss / d x[b][c] = (softmax(x[b])[c] * sum_c' t[b][c'] - t[b][c]) / B
// One wave per row: the row lives in registers (C <= 64 * 32), max and sums are DPP wave reductions, the gradient is
// written in the same pass.  Rows are summed to the scalar loss by a single-wave second kernel in a fixed order.
// The same row body serves the losses on integer labels (fv_label_ce: the target of a row is built in registers from
// labels[b] -- and, under batch-mode Mixup / CutMix, labels[B-1-b] and the mixing weights of the device parameter block --
// instead of read from a (B, C) tensor): timm's mixup_target + SoftTargetCrossEntropy, LabelSmoothingCrossEntropy,
// torch.nn.CrossEntropyLoss (supervised_imagenet.py:80-92), and the validation step's top-1 count.
#include "common.h"
#include "ce_row.h"

namespace {

// EPL, the two target sources and soft_ce_row_body: csrc/ce_row.h (csrc/eval.hip runs the same row body)
using namespace fv_ce_row;

template <typename T>
__global__ __launch_bounds__(256) void soft_ce_rows_kernel(const T* __restrict__ x, const float* __restrict__ t,
                                                            float* __restrict__ loss_rows, float* __restrict__ dx, int B,
                                                            int C, float inv_b) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= B) return;
  const DenseTarget ts{t + (size_t)row * C, 0};
  soft_ce_row_body<T>(x + (size_t)row * C, ts, loss_rows, dx, nullptr, row, C, inv_b);
}

// The same rows with the target built from labels[b] (and, MIX, labels[B-1-b] and the mix-parameter block, read here at
// run time: a captured launch picks up what the host wrote into the block since the last replay).
template <typename T, bool MIX>
__global__ __launch_bounds__(256) void label_ce_rows_kernel(const T* __restrict__ x, const int64_t* __restrict__ labels,
                                                             const fv_mix_params* __restrict__ mp, float on, float off,
                                                             float* __restrict__ loss_rows, float* __restrict__ dx,
                                                             int32_t* __restrict__ correct_rows, int B, int C, float inv_b) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= B) return;
  LabelTarget<MIX> ts;
  ts.label = labels[row];
  ts.partner = MIX ? labels[B - 1 - row] : -1;
  ts.on = on; ts.off = off;
  ts.lam = MIX ? mp->lam : 1.f;
  ts.oml = MIX ? mp->one_minus_lam : 0.f;
  soft_ce_row_body<T>(x + (size_t)row * C, ts, loss_rows, dx, correct_rows, row, C, inv_b);
}

// target[b][c] for the drop-in Mixup.__call__: one thread per element
__global__ __launch_bounds__(256) void mixup_target_kernel(const int64_t* __restrict__ labels, const fv_mix_params* __restrict__ mp,
                                                           float on, float off, float* __restrict__ target, int B, int C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * C) return;
  const int b = i / C, c = i - b * C;
  target[i] = mix_target_value(c, labels[b], labels[B - 1 - b], on, off, mp->lam, mp->one_minus_lam);
}

// loss = inv_b * sum_b loss_rows[b], one wave, fixed order (lane-strided partial sums, then the butterfly); the count of
// correct rows the same way
__global__ __launch_bounds__(64) void soft_ce_mean_kernel(const float* __restrict__ loss_rows, float* __restrict__ loss,
                                                          int B, float inv_b, const int32_t* __restrict__ correct_rows,
                                                          int32_t* __restrict__ n_correct) {
  float s = 0.f;
  for (int b = threadIdx.x; b < B; b += 64) s += loss_rows[b];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (threadIdx.x == 0) loss[0] = s * inv_b;
  if (correct_rows && n_correct) {
    int n = 0;
    for (int b = threadIdx.x; b < B; b += 64) n += correct_rows[b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if (threadIdx.x == 0) n_correct[0] = n;
  }
}

// off = smoothing / classes, on = 1 - smoothing + off as Python evaluates them: IEEE double operations in source order
// (the volatiles keep -ffast-math from re-associating them or dividing by a reciprocal), each rounded to fp32 once
void smoothing_values(double smoothing, int classes, float* on, float* off) {
  volatile double s = smoothing, c = (double)classes;
  volatile double offd = s / c;
  volatile double t = 1.0 - s;
  volatile double ond = t + offd;
  *off = (float)offd;
  *on = (float)ond;
}

}  // namespace

extern "C" int fv_soft_target_ce(const void* logits, int logits_dtype, const float* target, float* loss_rows, float* loss,
                                 float* dlogits, int batch, int classes, fv_stream_t stream) {
  FV_CHECK(logits && target && loss_rows && loss && dlogits, "soft_target_ce: null pointer");
  FV_CHECK(batch > 0 && classes > 0, "soft_target_ce: empty dimension");
  FV_CHECK(classes <= 64 * EPL, "soft_target_ce: at most %d classes (got %d)", 64 * EPL, classes);
  FV_CHECK(logits_dtype == FV_F32 || logits_dtype == FV_BF16, "soft_target_ce: logits must be fp32 or bf16");
  hipStream_t st = (hipStream_t)stream;
  const float inv_b = 1.f / (float)batch;
  const dim3 grid(fv_cdiv(batch, 4)), block(256);
  if (logits_dtype == FV_F32)
    hipLaunchKernelGGL(soft_ce_rows_kernel<float>, grid, block, 0, st, (const float*)logits, target, loss_rows, dlogits, batch, classes, inv_b);
  else
    hipLaunchKernelGGL(soft_ce_rows_kernel<bf16_t>, grid, block, 0, st, (const bf16_t*)logits, target, loss_rows, dlogits, batch, classes, inv_b);
  hipLaunchKernelGGL(soft_ce_mean_kernel, dim3(1), dim3(64), 0, st, loss_rows, loss, batch, inv_b, (const int32_t*)nullptr, (int32_t*)nullptr);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_mixup_target(const int64_t* labels, float* target, int batch, int classes, double smoothing, const void* mix,
                               fv_stream_t stream) {
  FV_CHECK(labels && target && mix, "mixup_target: null pointer");
  FV_CHECK(batch > 0 && classes > 0 && (long)batch * classes < (1l << 31), "mixup_target: bad shape (%d, %d)", batch, classes);
  FV_CHECK(batch % 2 == 0, "mixup_target: batch mode pairs sample b with batch-1-b, the batch (%d) must be even", batch);
  FV_CHECK(smoothing >= 0.0 && smoothing < 1.0, "mixup_target: smoothing must be in [0, 1)");
  float on, off;
  smoothing_values(smoothing, classes, &on, &off);
  hipLaunchKernelGGL(mixup_target_kernel, dim3(fv_cdiv((long)batch * classes, 256)), dim3(256), 0, (hipStream_t)stream, labels,
                     (const fv_mix_params*)mix, on, off, target, batch, classes);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_label_ce(const void* logits, int logits_dtype, const int64_t* labels, const void* mix, double smoothing,
                           float* loss_rows, float* loss, float* dlogits, int32_t* correct_rows, int32_t* n_correct, int batch,
                           int classes, fv_stream_t stream) {
  FV_CHECK(logits && labels && loss_rows && loss, "label_ce: null pointer");
  FV_CHECK(batch > 0 && classes > 0, "label_ce: empty dimension");
  FV_CHECK(classes <= 64 * EPL, "label_ce: at most %d classes (got %d)", 64 * EPL, classes);
  FV_CHECK(logits_dtype == FV_F32 || logits_dtype == FV_BF16, "label_ce: logits must be fp32 or bf16");
  FV_CHECK(!mix || batch % 2 == 0, "label_ce: batch mode pairs sample b with batch-1-b, the batch (%d) must be even", batch);
  FV_CHECK(smoothing >= 0.0 && smoothing < 1.0, "label_ce: smoothing must be in [0, 1)");
  FV_CHECK((correct_rows != nullptr) == (n_correct != nullptr), "label_ce: correct_rows and n_correct come together");
  float on, off;
  smoothing_values(smoothing, classes, &on, &off);
  hipStream_t st = (hipStream_t)stream;
  const float inv_b = 1.f / (float)batch;
  const dim3 grid(fv_cdiv(batch, 4)), block(256);
  const fv_mix_params* mp = (const fv_mix_params*)mix;
#define FV_LCE(T, MIX) hipLaunchKernelGGL((label_ce_rows_kernel<T, MIX>), grid, block, 0, st, (const T*)logits, labels, mp, on, off, loss_rows, dlogits, correct_rows, batch, classes, inv_b)
  if (logits_dtype == FV_F32) { if (mp) FV_LCE(float, true); else FV_LCE(float, false); }
  else { if (mp) FV_LCE(bf16_t, true); else FV_LCE(bf16_t, false); }
#undef FV_LCE
  hipLaunchKernelGGL(soft_ce_mean_kernel, dim3(1), dim3(64), 0, st, loss_rows, loss, batch, inv_b, (const int32_t*)correct_rows, n_correct);
  FV_LAUNCH_CHECK();
  return FV_OK;
}
