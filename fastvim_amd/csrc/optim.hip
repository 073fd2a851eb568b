// Fused AdamW over the flat parameter buffer (+ optional EMA of the weights, + bf16 shadow refresh).
// Replaces, per training step of the reference (imagenet_classification/supervised_imagenet.py:134-147,
// 270-276): torch.optim.AdamW over two parameter groups, ModelEmaV2.update (a full-parameter lerp) and
// the per-layer autocast weight casts -- ~20 multi-tensor launches + 6 casts per block -- by ONE
// HBM-bound pass: 16 B read + 14 B written per parameter (+ 8 B with EMA).
// `lr` and `step` live in device memory so a captured HIP graph replays with a changing schedule.
//
// The fine-tune recipe of the reference (mae/finetune_imagenet.py:238-262, mae/lr_decay.py; gradient_clip_val of
// mae/config/finetune_FastVimH_448.yaml) needs per-group learning rates and a clip of the global gradient norm:
//   grad_sumsq_kernel          one fp32 partial sum of squares of the raw gradient per workgroup (no atomics, no counter)
//   adamw_flat_groups_kernel   the same single pass with a group byte per element in place of the decay byte, a device
//                              table of (lr_scale, weight_decay) per group, and -- when partials are given -- every
//                              workgroup finishing the partials in one fixed order to get the clip coefficient
#include "common.h"
#include "lane_reduce.h"

namespace {

struct AdamParams {
  float *p, *m, *v, *ema;
  const float* g;
  bf16_t* shadow;
  const uint8_t* decay_mask;   // 1 = apply weight decay
  const float* lr;             // device scalar
  float* step;                 // device scalar (float), incremented by this launch
  float beta1, beta2, eps, weight_decay, ema_decay;
  float grad_scale;            // every gradient element is multiplied by this as it is read (1 / world size after a sum all-reduce)
  size_t n;
};

// The per-element AdamW update, shared by adamw_flat_kernel and adamw_flat_groups_kernel so that the two cannot drift.
// The library is built with -ffast-math, under which the compiler picks the association and the fused pairs of a
// plain expression per kernel (the same source line came out as different roundings in two kernels).  So the update is
// written operation by operation -- explicit fma where a product is fused, `rounded()` where a product must NOT be fused
// into the addition that follows (the backend fuses across statements under -ffast-math, whatever the pragma says) -- in
// exactly the form the plain expression of adamw_flat_kernel compiled to (read off the gfx950 ISA that hipcc of ROCm
// 7.2.0, AMD clang 22, made of it with this library's flags; the results are bit-identical to that build's):
//   gs = g * gmul                                   (gmul = grad_scale [* clip coefficient])
//   p  = decay ? p * (1 - lr * weight_decay) : p    (decay_factor, one fma, is passed in)
//   m  = beta1 * (m - g * gmul) + gs                (== beta1 m + (1 - beta1) gs; the inner product is fused)
//   v  = beta2 * (v - gs^2) + gs^2
//   p -= (m * lr) / ((sqrt(v) / sqrt(bc2) + eps) * bc1)        (hardware sqrt and reciprocal, 1 ulp each)
__device__ __forceinline__ float rounded(float x) {
  asm("" : "+v"(x));          // an opaque copy: what is computed from it cannot be merged with what computed it
  return x;
}
__device__ __forceinline__ void adamw_element(float& p, float& m, float& v, float g, float gmul, bool decay,
                                              float decay_factor, float lr, float bc1, float beta1, float beta2,
                                              float eps, float inv_sqrt_bc2) {
#pragma clang fp reassociate(off) contract(off)
  const float gs = g * gmul;
  const float pd = decay ? rounded(p * decay_factor) : p;      // decoupled weight decay
  m = __builtin_fmaf(__builtin_fmaf(-g, gmul, m), beta1, gs);
  v = __builtin_fmaf(__builtin_fmaf(-gs, gs, v), beta2, gs * gs);
  const float den = __builtin_fmaf(__builtin_amdgcn_sqrtf(v), inv_sqrt_bc2, eps) * bc1;
  p = pd - rounded((m * lr) * __builtin_amdgcn_rcpf(den));
}

// 1 - lr * weight_decay, one rounding
__device__ __forceinline__ float adamw_decay_factor(float lr, float weight_decay) {
  return __builtin_fmaf(-lr, weight_decay, 1.f);
}

// Write back 4 updated elements at offset i: masters and moments, the bf16 shadow, the EMA of the weights
// (ema = (1 - d) * p + ema * d: the second product rounded, then one fma).
__device__ __forceinline__ void adamw_store4(float* P, float* M, float* V, bf16_t* shadow, float* ema, float ema_decay,
                                             size_t i, float4 p, float4 m, float4 v) {
#pragma clang fp reassociate(off) contract(off)
  *reinterpret_cast<float4*>(P + i) = p;
  *reinterpret_cast<float4*>(M + i) = m;
  *reinterpret_cast<float4*>(V + i) = v;
  if (shadow) {
    uint2 pk = {pack_bf16x2(p.x, p.y), pack_bf16x2(p.z, p.w)};
    *reinterpret_cast<uint2*>(shadow + i) = pk;
  }
  if (ema) {
    const float om = 1.f - ema_decay;
    float4 e4 = *reinterpret_cast<const float4*>(ema + i);
    e4.x = __builtin_fmaf(p.x, om, e4.x * ema_decay);
    e4.y = __builtin_fmaf(p.y, om, e4.y * ema_decay);
    e4.z = __builtin_fmaf(p.z, om, e4.z * ema_decay);
    e4.w = __builtin_fmaf(p.w, om, e4.w * ema_decay);
    *reinterpret_cast<float4*>(ema + i) = e4;
  }
}

__global__ __launch_bounds__(256) void adamw_flat_kernel(AdamParams a) {
  const float t = a.step[0] + 1.f;                     // every thread reads the pre-increment value
  const float lr = a.lr[0];
  const float bc1 = 1.f - __powf(a.beta1, t), bc2 = 1.f - __powf(a.beta2, t);
  const float inv_sqrt_bc2 = rsqrtf(bc2);
  const float decay_factor = adamw_decay_factor(lr, a.weight_decay);
  const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
  for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < a.n; i += stride) {
    float4 p = *reinterpret_cast<const float4*>(a.p + i);
    const float4 g = *reinterpret_cast<const float4*>(a.g + i);
    float4 m = *reinterpret_cast<const float4*>(a.m + i);
    float4 v = *reinterpret_cast<const float4*>(a.v + i);
    const uint32_t mask = *reinterpret_cast<const uint32_t*>(a.decay_mask + i);
    float* pp = &p.x; const float* gg = &g.x; float* mm = &m.x; float* vv = &v.x;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      adamw_element(pp[e], mm[e], vv[e], gg[e], a.grad_scale, (mask >> (8 * e)) & 1u, decay_factor, lr, bc1,
                    a.beta1, a.beta2, a.eps, inv_sqrt_bc2);
    adamw_store4(a.p, a.m, a.v, a.shadow, a.ema, a.ema_decay, i, p, m, v);
  }
}

__global__ void bump_step_kernel(float* step) { step[0] += 1.f; }

// ------------------------------------------------------------------------------------------------ gradient norm
// Sum over the 64 lanes of a wave, every lane returning the same bits: cross-row swaps for lane bits 5 and 4
// (v_permlane32_swap / v_permlane16_swap), DPP row rotates for bits 3 and 2, quad permutes for bits 1 and 0.  Each level
// adds a lane's value and its partner's, so both sides of a pair compute the same sum (addition commutes).  6 additions.
__device__ __forceinline__ float wave_allsum(float v) {
#pragma clang fp reassociate(off) contract(off)
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  v = add_dpp<0x128>(v);       // row_ror:8 == lane ^ 8
  v = add_dpp<0x124>(v);       // row_ror:4: the values have period 8 inside a row by now, so this is lane ^ 4
  return quad_sum(v);
}

constexpr int kSumsqThreads = 256;                       // 4 waves
constexpr int kSumsqQuads = 4;                           // independent 16-byte loads (and float4 accumulators) per lane and trip
constexpr int kSumsqMaxBlocks = 1024;                    // = 256 threads x one float4: the consumer's prologue is ONE load per lane
constexpr int kSumsqTile = kSumsqThreads * kSumsqQuads;  // float4 per workgroup and trip

// Sum of the 4 waves' values through LDS, in one fixed order, the same bits in every thread.  2 additions.
__device__ __forceinline__ float block_allsum4(float wave_total, float* s_w) {
#pragma clang fp reassociate(off) contract(off)
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) s_w[tid >> 6] = wave_total;
  __syncthreads();
  return (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// partials[blockIdx.x] = sum of g[i]^2 over the workgroup's float4 tiles.  n4 = n / 4.
// Longest chain of dependent additions: trips (one fma per accumulator and trip) + 4 (16 accumulators of a lane, as a
// tree) + 6 (wave) + 2 (4 waves).
__global__ __launch_bounds__(kSumsqThreads) void grad_sumsq_kernel(const float* __restrict__ g, float* __restrict__ partials,
                                                                   size_t n4) {
#pragma clang fp reassociate(off) contract(off)
  __shared__ float s_w[4];
  const float4* g4 = reinterpret_cast<const float4*>(g);
  float4 acc[kSumsqQuads];
#pragma unroll
  for (int u = 0; u < kSumsqQuads; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
  const size_t stride = (size_t)gridDim.x * kSumsqTile;
  for (size_t b = (size_t)blockIdx.x * kSumsqTile + threadIdx.x; b < n4; b += stride) {
    float4 x[kSumsqQuads];
    if (b + (kSumsqQuads - 1) * kSumsqThreads < n4) {
#pragma unroll
      for (int u = 0; u < kSumsqQuads; ++u) x[u] = g4[b + u * kSumsqThreads];
    } else {
#pragma unroll
      for (int u = 0; u < kSumsqQuads; ++u)
        x[u] = b + u * kSumsqThreads < n4 ? g4[b + u * kSumsqThreads] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < kSumsqQuads; ++u) {
      acc[u].x = __builtin_fmaf(x[u].x, x[u].x, acc[u].x);
      acc[u].y = __builtin_fmaf(x[u].y, x[u].y, acc[u].y);
      acc[u].z = __builtin_fmaf(x[u].z, x[u].z, acc[u].z);
      acc[u].w = __builtin_fmaf(x[u].w, x[u].w, acc[u].w);
    }
  }
  const float sx = (acc[0].x + acc[1].x) + (acc[2].x + acc[3].x);
  const float sy = (acc[0].y + acc[1].y) + (acc[2].y + acc[3].y);
  const float sz = (acc[0].z + acc[1].z) + (acc[2].z + acc[3].z);
  const float sw = (acc[0].w + acc[1].w) + (acc[2].w + acc[3].w);
  const float total = block_allsum4(wave_allsum((sx + sy) + (sz + sw)), s_w);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// The consumer's side: a 256-thread workgroup sums the G <= 1024 partials (4 per lane, 16-byte load where all 4 exist),
// in one fixed order, so every workgroup of every launch that calls this holds the same bits.  2 + 6 + 2 additions.
__device__ __forceinline__ float finish_partials(const float* __restrict__ partials, int G, float* s_w) {
#pragma clang fp reassociate(off) contract(off)
  const int j = threadIdx.x * 4;
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
  if (j + 3 < G) {
    q = *reinterpret_cast<const float4*>(partials + j);
  } else {
    if (j < G) q.x = partials[j];
    if (j + 1 < G) q.y = partials[j + 1];
    if (j + 2 < G) q.z = partials[j + 2];
  }
  return block_allsum4(wave_allsum((q.x + q.y) + (q.z + q.w)), s_w);
}

__device__ __forceinline__ bool is_finite_f32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

struct AdamGroupParams {
  float *p, *m, *v, *ema;
  const float* g;
  bf16_t* shadow;
  const uint8_t* group_ids;    // one byte per element: row of `table`
  const float* table;          // n_groups x (lr_scale, weight_decay)
  const float* lr;             // device scalar: the base lr
  float* step;
  const float* partials;       // n_partials sums of squares of the raw gradient, or null: no clip, no skip
  const float* max_norm;       // device scalar, or null: no clip
  float* stats;                // [total_norm, clip_coef, finite, skipped_steps]
  float beta1, beta2, eps, ema_decay, grad_scale;
  int n_groups, n_partials, skip_nonfinite;
  size_t n;
};

__global__ __launch_bounds__(256) void adamw_flat_groups_kernel(AdamGroupParams a) {
  __shared__ float2 s_tab[256];          // per group: (lr_g, 1 - lr_g * weight_decay_g)
  __shared__ float s_w[4];
  const int tid = threadIdx.x;
  const float t = a.step[0] + 1.f;                     // every thread reads the pre-increment value
  const float lr = a.lr[0];
  const float bc1 = 1.f - __powf(a.beta1, t), bc2 = 1.f - __powf(a.beta2, t);
  const float inv_sqrt_bc2 = rsqrtf(bc2);
  float gmul = a.grad_scale;
  if (a.partials) {
    const float sum = finish_partials(a.partials, a.n_partials, s_w);       // bit-identical in every workgroup
    const bool finite = is_finite_f32(sum);
    const float total_norm = a.grad_scale * (float)sqrt((double)sum);      // (the root correctly rounded to fp32)
    float coef = 1.f;
    if (a.max_norm) {
      const float c = a.max_norm[0] / (total_norm + 1e-6f);               // torch.nn.utils.clip_grad_norm_
      coef = c > 1.f ? 1.f : c;                                             // (a NaN norm stays a NaN coefficient, as there)
    }
    if (blockIdx.x == 0 && tid == 0) {
      a.stats[0] = total_norm;
      a.stats[1] = coef;
      a.stats[2] = finite ? 1.f : 0.f;
    }
    if (a.skip_nonfinite && !finite) return;           // uniform over the whole launch: nothing is touched
    gmul = a.grad_scale * coef;
  }
  {
    float2 e = make_float2(0.f, 1.f);                  // rows past the table: lr 0, no decay
    if (tid < a.n_groups) {
      const float lr_g = lr * a.table[2 * tid];
      e = make_float2(lr_g, adamw_decay_factor(lr_g, a.table[2 * tid + 1]));
    }
    s_tab[tid] = e;
  }
  __syncthreads();
  const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
  for (size_t i = ((size_t)blockIdx.x * blockDim.x + tid) * 4; i < a.n; i += stride) {
    float4 p = *reinterpret_cast<const float4*>(a.p + i);
    const float4 g = *reinterpret_cast<const float4*>(a.g + i);
    float4 m = *reinterpret_cast<const float4*>(a.m + i);
    float4 v = *reinterpret_cast<const float4*>(a.v + i);
    const uint32_t ids = *reinterpret_cast<const uint32_t*>(a.group_ids + i);
    float* pp = &p.x; const float* gg = &g.x; float* mm = &m.x; float* vv = &v.x;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float2 c = s_tab[(ids >> (8 * e)) & 255u];
      adamw_element(pp[e], mm[e], vv[e], gg[e], gmul, true, c.y, c.x, bc1, a.beta1, a.beta2, a.eps, inv_sqrt_bc2);
    }
    adamw_store4(a.p, a.m, a.v, a.shadow, a.ema, a.ema_decay, i, p, m, v);
  }
}

// After adamw_flat_groups_kernel, when it was given partials: ONE workgroup finishes the same partials the same way and
// either advances the step count or, for a skipped step, the count of skipped steps.  (The main pass reads step[0] and
// never the stats record; this launch follows it in stream order.)
__global__ __launch_bounds__(256) void bump_step_checked_kernel(float* step, float* stats, const float* partials,
                                                                int n_partials, int skip_nonfinite) {
  __shared__ float s_w[4];
  const float sum = finish_partials(partials, n_partials, s_w);
  if (threadIdx.x == 0) {
    if (skip_nonfinite && !is_finite_f32(sum)) stats[3] += 1.f;
    else step[0] += 1.f;
  }
}

}  // namespace

extern "C" int fv_adamw_flat(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema,
                             void* shadow_bf16, const uint8_t* decay_mask, const float* lr, float* step,
                             float beta1, float beta2, float eps, float weight_decay, float ema_decay, float grad_scale,
                             size_t n, fv_stream_t stream) {
  FV_CHECK(params && grads && exp_avg && exp_avg_sq && decay_mask && lr && step, "adamw_flat: null pointer");
  FV_CHECK(n % 4 == 0, "adamw_flat: element count must be a multiple of 4 (pad the flat buffer)");
  AdamParams a{};
  a.p = params; a.g = grads; a.m = exp_avg; a.v = exp_avg_sq; a.ema = ema; a.shadow = (bf16_t*)shadow_bf16;
  a.decay_mask = decay_mask; a.lr = lr; a.step = step;
  a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.weight_decay = weight_decay; a.ema_decay = ema_decay; a.grad_scale = grad_scale; a.n = n;
  if (n == 0) return FV_OK;
  long blocks = fv_cdiv((long)(n / 4), 256);
  if (blocks > 2048) blocks = 2048;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(adamw_flat_kernel, dim3((int)blocks), dim3(256), 0, st, a);
  hipLaunchKernelGGL(bump_step_kernel, dim3(1), dim3(1), 0, st, step);   // after: the main pass read the old value
  FV_LAUNCH_CHECK();
  return FV_OK;
}

// Workgroups (= partials) of the sum-of-squares launch over n floats: a pure function of n (never of the device), two
// trips per workgroup at least, at most 1024.
extern "C" int fv_grad_sumsq_blocks(size_t n) {
  const size_t n4 = n / 4;
  size_t g = (n4 + 2 * (size_t)kSumsqTile - 1) / (2 * (size_t)kSumsqTile);
  if (g < 1) g = 1;
  if (g > (size_t)kSumsqMaxBlocks) g = kSumsqMaxBlocks;
  return (int)g;
}

extern "C" int fv_grad_sumsq_partials(const float* grads, float* partials, size_t n, fv_stream_t stream) {
  FV_CHECK(grads && partials, "grad_sumsq_partials: null pointer");
  FV_CHECK(n % 4 == 0, "grad_sumsq_partials: element count must be a multiple of 4 (pad the flat buffer)");
  FV_CHECK(((uintptr_t)grads & 15) == 0, "grad_sumsq_partials: the gradient must be 16-byte aligned");
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(fv_grad_sumsq_blocks(n)), dim3(kSumsqThreads), 0, (hipStream_t)stream,
                     grads, partials, n / 4);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_adamw_flat_groups(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema,
                                    void* shadow_bf16, const uint8_t* group_ids, const float* group_table, int n_groups,
                                    const float* lr, float* step, const float* partials, int n_partials,
                                    const float* max_norm, float* stats, int skip_nonfinite, float beta1, float beta2,
                                    float eps, float ema_decay, float grad_scale, size_t n, fv_stream_t stream) {
  FV_CHECK(params && grads && exp_avg && exp_avg_sq && group_ids && group_table && lr && step,
           "adamw_flat_groups: null pointer");
  FV_CHECK(n % 4 == 0, "adamw_flat_groups: element count must be a multiple of 4 (pad the flat buffer)");
  FV_CHECK((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)ema) & 15) == 0 &&
               ((uintptr_t)shadow_bf16 & 7) == 0 && ((uintptr_t)group_ids & 3) == 0,
           "adamw_flat_groups: the flat buffers must be 16-byte aligned (shadow 8, group bytes 4)");
  FV_CHECK(n_groups >= 1 && n_groups <= 256, "adamw_flat_groups: 1 to 256 groups (a group byte per element), got %d", n_groups);
  if (partials) {
    FV_CHECK(n_partials == fv_grad_sumsq_blocks(n), "adamw_flat_groups: %d partials given, fv_grad_sumsq_blocks(n) = %d",
             n_partials, fv_grad_sumsq_blocks(n));
    FV_CHECK(((uintptr_t)partials & 15) == 0, "adamw_flat_groups: the partials buffer must be 16-byte aligned");
    FV_CHECK(stats, "adamw_flat_groups: partials given without a stats record");
  } else {
    FV_CHECK(!max_norm && !skip_nonfinite, "adamw_flat_groups: clipping / skipping needs the partials of fv_grad_sumsq_partials");
  }
  AdamGroupParams a{};
  a.p = params; a.g = grads; a.m = exp_avg; a.v = exp_avg_sq; a.ema = ema; a.shadow = (bf16_t*)shadow_bf16;
  a.group_ids = group_ids; a.table = group_table; a.lr = lr; a.step = step;
  a.partials = partials; a.max_norm = max_norm; a.stats = stats;
  a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.ema_decay = ema_decay; a.grad_scale = grad_scale;
  a.n_groups = n_groups; a.n_partials = n_partials; a.skip_nonfinite = skip_nonfinite ? 1 : 0; a.n = n;
  if (n == 0) return FV_OK;
  long blocks = fv_cdiv((long)(n / 4), 256);
  if (blocks > 2048) blocks = 2048;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(adamw_flat_groups_kernel, dim3((int)blocks), dim3(256), 0, st, a);
  if (partials)
    hipLaunchKernelGGL(bump_step_checked_kernel, dim3(1), dim3(256), 0, st, step, stats, partials, n_partials, a.skip_nonfinite);
  else
    hipLaunchKernelGGL(bump_step_kernel, dim3(1), dim3(1), 0, st, step);
  FV_LAUNCH_CHECK();
  return FV_OK;
}
