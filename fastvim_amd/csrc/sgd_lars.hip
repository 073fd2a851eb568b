// Momentum SGD and LARS over the flat parameter buffer (+ bf16 shadow refresh): the optimizers of the reference's
// linear-probe recipe (mae/linear_imagenet.py:230: torch.optim.SGD(momentum=0.9, weight_decay=0); mae/lars.py, the
// optimizer the recipe was derived with).  `lr` lives in device memory, as for the fused AdamW (optim.hip).
//
//   sgd_flat_kernel        g' = g * grad_scale + wd * p (where the decay byte is set); buf = momentum * buf + g';
//                          p -= lr * buf; shadow = bf16(p).  With a zero buffer: torch SGD, dampening 0, no Nesterov.
//   lars_sumsq_kernel      per segment (= parameter) kLarsParts fixed-order partial sums of |p|^2 and |g * grad_scale + wd * p|^2
//   lars_flat_kernel       every workgroup finishes the partials of ITS segment in one fixed order, forms
//                          q = trust * |p| / |dp| (1 where either norm is 0), and applies dp * q through the momentum
//                          buffer.  Segments with ndim <= 1 take neither weight decay nor q (lars.py:29).
//
// The segment table is device memory, three int64 per segment: (first element, element count, ndim > 1).  A segment that
// does not lie inside [0, n) is skipped by both kernels, whatever the table holds.
#include "common.h"

namespace {

struct SgdParams {
  float *p, *buf;
  const float* g;
  bf16_t* shadow;
  const uint8_t* decay_mask;
  const float* lr;
  float momentum, weight_decay, grad_scale;
  size_t n;
};

__device__ __forceinline__ void sgd_element(float& p, float& buf, float g, float gs, float wd, float momentum, float lr) {
#pragma clang fp reassociate(off) contract(off)
  const float gd = __builtin_fmaf(wd, p, g * gs);
  buf = __builtin_fmaf(momentum, buf, gd);
  p = __builtin_fmaf(-lr, buf, p);
}

__global__ __launch_bounds__(256) void sgd_flat_kernel(SgdParams a) {
  const float lr = a.lr[0];
  const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
  for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < a.n; i += stride) {
    float4 p = *reinterpret_cast<const float4*>(a.p + i);
    const float4 g = *reinterpret_cast<const float4*>(a.g + i);
    float4 b = *reinterpret_cast<const float4*>(a.buf + i);
    const uint32_t mask = *reinterpret_cast<const uint32_t*>(a.decay_mask + i);
    float* pp = &p.x; const float* gg = &g.x; float* bb = &b.x;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      sgd_element(pp[e], bb[e], gg[e], a.grad_scale, ((mask >> (8 * e)) & 1u) ? a.weight_decay : 0.f, a.momentum, lr);
    *reinterpret_cast<float4*>(a.p + i) = p;
    *reinterpret_cast<float4*>(a.buf + i) = b;
    if (a.shadow) {
      uint2 pk = {pack_bf16x2(p.x, p.y), pack_bf16x2(p.z, p.w)};
      *reinterpret_cast<uint2*>(a.shadow + i) = pk;
    }
  }
}

// ------------------------------------------------------------------------------------------------ LARS
constexpr int kLarsParts = 64;        // workgroups (= partials of each norm) per segment: one wave finishes them
constexpr int kLarsThreads = 256;

struct Segment { long long off, len, matrix; };

__device__ __forceinline__ bool load_segment(const int64_t* table, int s, size_t n, Segment& sg) {
  sg.off = table[3 * s]; sg.len = table[3 * s + 1]; sg.matrix = table[3 * s + 2];
  return sg.off >= 0 && sg.len > 0 && (unsigned long long)sg.off <= n && (unsigned long long)sg.len <= n - (size_t)sg.off;
}

// Sum over the 64 lanes: a butterfly (each level adds a lane's value and its partner's, so both hold the same bits).
__device__ __forceinline__ float wave_allsum_f(float v) {
#pragma clang fp reassociate(off) contract(off)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_allsum_d(double v) {
#pragma clang fp reassociate(off) contract(off)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}

// partials[(s * 2 + k) * kLarsParts + blockIdx.x], k = 0: |p|^2, k = 1: |g * grad_scale + wd * p|^2
__global__ __launch_bounds__(kLarsThreads) void lars_sumsq_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                                   const int64_t* __restrict__ table,
                                                                   float* __restrict__ partials, float wd, float gs, size_t n) {
#pragma clang fp reassociate(off) contract(off)
  __shared__ float s_w[2][4];
  const int s = blockIdx.y, tid = threadIdx.x;
  Segment sg;
  const bool ok = load_segment(table, s, n, sg);
  float ap[4] = {0.f, 0.f, 0.f, 0.f}, ad[4] = {0.f, 0.f, 0.f, 0.f};
  if (ok && sg.matrix) {
    const float* P = p + sg.off;
    const float* G = g + sg.off;
    const bool vec = (sg.off & 3) == 0;
    const long long quads = (sg.len + 3) / 4;
    for (long long q = (long long)blockIdx.x * kLarsThreads + tid; q < quads; q += (long long)kLarsParts * kLarsThreads) {
      float pv[4] = {0.f, 0.f, 0.f, 0.f}, gv[4] = {0.f, 0.f, 0.f, 0.f};
      if (vec && q * 4 + 3 < sg.len) {
        const float4 a = *reinterpret_cast<const float4*>(P + q * 4), b = *reinterpret_cast<const float4*>(G + q * 4);
        pv[0] = a.x; pv[1] = a.y; pv[2] = a.z; pv[3] = a.w;
        gv[0] = b.x; gv[1] = b.y; gv[2] = b.z; gv[3] = b.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (q * 4 + e < sg.len) { pv[e] = P[q * 4 + e]; gv[e] = G[q * 4 + e]; }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float dp = __builtin_fmaf(wd, pv[e], gv[e] * gs);
        ap[e] = __builtin_fmaf(pv[e], pv[e], ap[e]);
        ad[e] = __builtin_fmaf(dp, dp, ad[e]);
      }
    }
  }
  const float tp = wave_allsum_f((ap[0] + ap[1]) + (ap[2] + ap[3]));
  const float td = wave_allsum_f((ad[0] + ad[1]) + (ad[2] + ad[3]));
  if ((tid & 63) == 0) { s_w[0][tid >> 6] = tp; s_w[1][tid >> 6] = td; }
  __syncthreads();
  if (tid == 0) {
    partials[((size_t)s * 2 + 0) * kLarsParts + blockIdx.x] = (s_w[0][0] + s_w[0][1]) + (s_w[0][2] + s_w[0][3]);
    partials[((size_t)s * 2 + 1) * kLarsParts + blockIdx.x] = (s_w[1][0] + s_w[1][1]) + (s_w[1][2] + s_w[1][3]);
  }
}

struct LarsParams {
  float *p, *buf;
  const float* g;
  bf16_t* shadow;
  const int64_t* table;
  const float* partials;
  const float* lr;
  float* norms;              // per segment [|p|, |dp|, q], or null
  float momentum, weight_decay, trust, grad_scale;
  size_t n;
};

__global__ __launch_bounds__(kLarsThreads) void lars_flat_kernel(LarsParams a) {
#pragma clang fp reassociate(off) contract(off)
  const int s = blockIdx.y, tid = threadIdx.x;
  Segment sg;
  if (!load_segment(a.table, s, a.n, sg)) return;      // (uniform over the workgroup)
  const float lr = a.lr[0];
  float q = 1.f, wd = 0.f;
  if (sg.matrix) {
    // every wave of every workgroup of the segment sums the same 64 partials in the same order (the roots correctly rounded)
    const float* part = a.partials + (size_t)s * 2 * kLarsParts;
    const double sp = wave_allsum_d((double)part[tid & 63]);
    const double sd = wave_allsum_d((double)part[kLarsParts + (tid & 63)]);
    const float pn = (float)sqrt(sp), un = (float)sqrt(sd);
    q = (pn > 0.f && un > 0.f) ? a.trust * pn / un : 1.f;
    wd = a.weight_decay;
    if (a.norms && blockIdx.x == 0 && tid == 0) {
      a.norms[3 * s] = pn; a.norms[3 * s + 1] = un; a.norms[3 * s + 2] = q;
    }
  } else if (a.norms && blockIdx.x == 0 && tid == 0) {
    a.norms[3 * s] = 0.f; a.norms[3 * s + 1] = 0.f; a.norms[3 * s + 2] = 1.f;
  }
  float* P = a.p + sg.off;
  float* M = a.buf + sg.off;
  const float* G = a.g + sg.off;
  bf16_t* S = a.shadow ? a.shadow + sg.off : nullptr;
  const bool vec = (sg.off & 3) == 0;
  const long long quads = (sg.len + 3) / 4;
  for (long long k = (long long)blockIdx.x * kLarsThreads + tid; k < quads; k += (long long)gridDim.x * kLarsThreads) {
    const long long i = k * 4;
    if (vec && i + 3 < sg.len) {
      float4 p = *reinterpret_cast<const float4*>(P + i);
      const float4 g = *reinterpret_cast<const float4*>(G + i);
      float4 m = *reinterpret_cast<const float4*>(M + i);
      float* pp = &p.x; const float* gg = &g.x; float* mm = &m.x;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float dp = __builtin_fmaf(wd, pp[e], gg[e] * a.grad_scale) * q;
        mm[e] = __builtin_fmaf(a.momentum, mm[e], dp);
        pp[e] = __builtin_fmaf(-lr, mm[e], pp[e]);
      }
      *reinterpret_cast<float4*>(P + i) = p;
      *reinterpret_cast<float4*>(M + i) = m;
      if (S) {
        uint2 pk = {pack_bf16x2(p.x, p.y), pack_bf16x2(p.z, p.w)};
        *reinterpret_cast<uint2*>(S + i) = pk;
      }
    } else {
      for (int e = 0; e < 4 && i + e < sg.len; ++e) {
        const float dp = __builtin_fmaf(wd, P[i + e], G[i + e] * a.grad_scale) * q;
        const float m = __builtin_fmaf(a.momentum, M[i + e], dp);
        const float p = __builtin_fmaf(-lr, m, P[i + e]);
        M[i + e] = m;
        P[i + e] = p;
        if (S) io<bf16_t>::st(S + i + e, p);
      }
    }
  }
}

}  // namespace

extern "C" int fv_sgd_flat(float* params, const float* grads, float* momentum_buf, void* shadow_bf16,
                           const uint8_t* decay_mask, const float* lr, float momentum, float weight_decay,
                           float grad_scale, size_t n, fv_stream_t stream) {
  FV_CHECK(params && grads && momentum_buf && decay_mask && lr, "sgd_flat: null pointer");
  FV_CHECK(n % 4 == 0, "sgd_flat: element count must be a multiple of 4 (pad the flat buffer)");
  FV_CHECK((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)momentum_buf) & 15) == 0 && ((uintptr_t)shadow_bf16 & 7) == 0 &&
               ((uintptr_t)decay_mask & 3) == 0,
           "sgd_flat: the flat buffers must be 16-byte aligned (shadow 8, decay bytes 4)");
  if (n == 0) return FV_OK;
  SgdParams a{};
  a.p = params; a.g = grads; a.buf = momentum_buf; a.shadow = (bf16_t*)shadow_bf16; a.decay_mask = decay_mask; a.lr = lr;
  a.momentum = momentum; a.weight_decay = weight_decay; a.grad_scale = grad_scale; a.n = n;
  long blocks = fv_cdiv((long)(n / 4), 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(sgd_flat_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, a);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_lars_partials_per_segment(void) { return kLarsParts; }

extern "C" int fv_lars_sumsq_partials(const float* params, const float* grads, const int64_t* segments, int n_segments,
                                      float* partials, float weight_decay, float grad_scale, size_t n, fv_stream_t stream) {
  FV_CHECK(params && grads && segments && partials, "lars_sumsq_partials: null pointer");
  FV_CHECK(n_segments >= 1 && n_segments <= 65535, "lars_sumsq_partials: 1 to 65535 segments, got %d", n_segments);
  FV_CHECK((((uintptr_t)params | (uintptr_t)grads) & 15) == 0, "lars_sumsq_partials: the flat buffers must be 16-byte aligned");
  hipLaunchKernelGGL(lars_sumsq_kernel, dim3(kLarsParts, n_segments), dim3(kLarsThreads), 0, (hipStream_t)stream, params,
                     grads, segments, partials, weight_decay, grad_scale, n);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_lars_flat(float* params, const float* grads, float* momentum_buf, void* shadow_bf16,
                            const int64_t* segments, int n_segments, const float* partials, const float* lr,
                            float* norms, float momentum, float weight_decay, float trust_coefficient, float grad_scale,
                            size_t n, fv_stream_t stream) {
  FV_CHECK(params && grads && momentum_buf && segments && partials && lr, "lars_flat: null pointer");
  FV_CHECK(n_segments >= 1 && n_segments <= 65535, "lars_flat: 1 to 65535 segments, got %d", n_segments);
  FV_CHECK((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)momentum_buf) & 15) == 0 && ((uintptr_t)shadow_bf16 & 7) == 0,
           "lars_flat: the flat buffers must be 16-byte aligned (shadow 8)");
  LarsParams a{};
  a.p = params; a.g = grads; a.buf = momentum_buf; a.shadow = (bf16_t*)shadow_bf16; a.table = segments;
  a.partials = partials; a.lr = lr; a.norms = norms;
  a.momentum = momentum; a.weight_decay = weight_decay; a.trust = trust_coefficient; a.grad_scale = grad_scale; a.n = n;
  hipLaunchKernelGGL(lars_flat_kernel, dim3(kLarsParts, n_segments), dim3(kLarsThreads), 0, (hipStream_t)stream, a);
  FV_LAUNCH_CHECK();
  return FV_OK;
}
