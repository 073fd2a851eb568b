// BatchNorm1d over pooled features (B, d) -- the linear-probe head of the reference (mae/linear_imagenet.py:39-53:
// Sequential(BatchNorm1d(d, affine=False, eps=1e-6), head); SyncBatchNorm under mae/linear.py:41).
//
//   bn1d_stats_kernel   per-column mean and centred sum of squares M2 of this rank's rows, as one table row
//                       [mean(d) | M2(d) | count].  Exact passes over the strip: the mean, its refinement by the mean of
//                       the deviations (so the stored mean is the correctly rounded one even where |mean| >> std), then the
//                       squared deviations from it -- never E[x^2] - E[x]^2.
//   bn1d_apply_kernel   merges `world` table rows in rank order (parallel-variance formula), writes xhat, the batch mean /
//                       rstd for the adjoint, and -- exactly one workgroup per column strip, one thread for the counter --
//                       the running buffers; eval mode normalises with the running statistics and writes no buffer.
//   bn1d_bwd_kernel     dx = rstd * (dy - mean_B(dy) - xhat * mean_B(dy * xhat)), column sums taken like the forward ones.
//
// Geometry of the two reducing kernels: a workgroup owns a strip of 64 contiguous columns (lane = column, so a wave reads
// one 128 / 256-byte run per row) and its 16 waves take rows w, w + 16, ...; the waves' values are combined through LDS in
// one fixed tree.  No atomics; the same input gives the same bits.
#include "common.h"

namespace {

constexpr int kStrip = 64;            // columns per workgroup = lanes of a wave
constexpr int kWaves = 16;            // waves (row groups) per workgroup of the reducing kernels
constexpr int kRegRows = 32;          // rows a lane keeps in registers: batches up to kWaves * kRegRows = 512 are read ONCE

// Sum of the 16 waves' per-column values, the same bits in every thread of a column.  One fixed tree.
__device__ __forceinline__ float strip_allsum(float v, float (*s_part)[kStrip], float* s_res) {
#pragma clang fp reassociate(off) contract(off)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();                    // (s_res of the previous call has been read by everyone)
  s_part[w][lane] = v;
  __syncthreads();
  if (w == 0) {
    float t[kWaves];
#pragma unroll
    for (int i = 0; i < kWaves; ++i) t[i] = s_part[i][lane];
#pragma unroll
    for (int h = kWaves / 2; h > 0; h >>= 1)
#pragma unroll
      for (int i = 0; i < h; ++i) t[i] = t[i] + t[i + h];
    s_res[lane] = t[0];
  }
  __syncthreads();
  return s_res[lane];
}

// fixed tree over the kRegRows register values of a lane
__device__ __forceinline__ float tree_sum(float (&t)[kRegRows]) {
#pragma clang fp reassociate(off) contract(off)
#pragma unroll
  for (int h = kRegRows / 2; h > 0; h >>= 1)
#pragma unroll
    for (int i = 0; i < h; ++i) t[i] = t[i] + t[i + h];
  return t[0];
}

// REG: the lane's rows stay in registers between the passes (B <= 512); otherwise every pass re-reads them (L2-resident:
// a strip is B x 256 bytes), 8 independent accumulators per lane.
template <typename T, bool REG>
__global__ __launch_bounds__(kStrip * kWaves) void bn1d_stats_kernel(const T* __restrict__ x, float* __restrict__ row,
                                                                      int B, int d) {
#pragma clang fp reassociate(off) contract(off)
  __shared__ float s_part[kWaves][kStrip];
  __shared__ float s_res[kStrip];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = blockIdx.x * kStrip + lane;
  const bool cok = col < d;
  const float invB = 1.f / (float)B;
  float mean, m2;
  if (REG) {
    float xr[kRegRows];
#pragma unroll
    for (int i = 0; i < kRegRows; ++i) {          // every load of the strip is in flight before the first add
      const int r = w + i * kWaves;
      xr[i] = (cok && r < B) ? io<T>::ld(x + (size_t)r * d + col) : 0.f;
    }
    float t[kRegRows];
#pragma unroll
    for (int i = 0; i < kRegRows; ++i) t[i] = xr[i];
    const float mean1 = strip_allsum(tree_sum(t), s_part, s_res) * invB;
#pragma unroll
    for (int i = 0; i < kRegRows; ++i) t[i] = (w + i * kWaves < B) ? xr[i] - mean1 : 0.f;
    mean = mean1 + strip_allsum(tree_sum(t), s_part, s_res) * invB;
#pragma unroll
    for (int i = 0; i < kRegRows; ++i) {
      const float dv = (w + i * kWaves < B) ? xr[i] - mean : 0.f;
      t[i] = dv * dv;
    }
    m2 = strip_allsum(tree_sum(t), s_part, s_res);
  } else {
    float acc[8];
    auto pass = [&](auto f) {
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u] = 0.f;
      for (int r0 = w; r0 < B; r0 += 8 * kWaves) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int r = r0 + u * kWaves;
          v[u] = (cok && r < B) ? io<T>::ld(x + (size_t)r * d + col) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] = acc[u] + ((r0 + u * kWaves < B) ? f(v[u]) : 0.f);
      }
      const float s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
      return strip_allsum(s, s_part, s_res);
    };
    const float mean1 = pass([](float v) { return v; }) * invB;
    mean = mean1 + pass([mean1](float v) { return v - mean1; }) * invB;
    const float mu = mean;
    m2 = pass([mu](float v) { const float dv = v - mu; return dv * dv; });
  }
  if (w == 0 && cok) {
    row[col] = mean;
    row[d + col] = m2;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) row[2 * (size_t)d] = (float)B;
}

struct BnApply {
  const void* x;
  void* xhat;
  const float* table;       // world rows of 2 d + 1 floats
  float *running_mean, *running_var;
  long long* num_batches_tracked;
  float *mean_out, *rstd_out;
  int world, B, d, training;
  float eps, momentum;
};

constexpr int kApplyRows = 32;        // rows per workgroup of the apply launch (4 waves x 8 rows)

template <typename T>
__global__ __launch_bounds__(256) void bn1d_apply_kernel(BnApply a) {
#pragma clang fp reassociate(off) contract(off)
  __shared__ float s_mean[kStrip], s_rstd[kStrip];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = blockIdx.x * kStrip + lane;
  const bool cok = col < a.d;
  const bool owner = blockIdx.y == 0;          // the ONE workgroup of this strip that writes statistics
  if (w == 0) {
    float mean = 0.f, rstd = 0.f;
    if (cok) {
      if (a.training) {
        const size_t stride = 2 * (size_t)a.d + 1;
        float n = a.table[2 * (size_t)a.d];
        mean = a.table[col];
        float m2 = a.table[a.d + col];
        for (int r = 1; r < a.world; ++r) {      // rank order: Chan et al.'s pairwise merge
          const float* t = a.table + r * stride;
          const float nb = t[2 * (size_t)a.d], mb = t[col], m2b = t[a.d + col];
          const float nn = n + nb, delta = mb - mean;
          mean = mean + delta * (nb / nn);
          m2 = (m2 + m2b) + (delta * delta) * (n * (nb / nn));
          n = nn;
        }
        const float var = m2 / n;
        rstd = 1.f / __builtin_sqrtf(var + a.eps);
        if (owner && a.running_mean) {
          const float unbiased = n > 1.f ? m2 / (n - 1.f) : var;
          a.running_mean[col] = (1.f - a.momentum) * a.running_mean[col] + a.momentum * mean;
          a.running_var[col] = (1.f - a.momentum) * a.running_var[col] + a.momentum * unbiased;
        }
      } else {
        mean = a.running_mean[col];
        rstd = 1.f / __builtin_sqrtf(a.running_var[col] + a.eps);
      }
      if (owner) {
        a.mean_out[col] = mean;
        a.rstd_out[col] = rstd;
      }
    }
    s_mean[lane] = mean;
    s_rstd[lane] = rstd;
  }
  if (a.training && a.num_batches_tracked && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
    a.num_batches_tracked[0] += 1;
  __syncthreads();
  if (!cok) return;
  const float mean = s_mean[lane], rstd = s_rstd[lane];
  const T* x = static_cast<const T*>(a.x);
  T* y = static_cast<T*>(a.xhat);
  const int r0 = blockIdx.y * kApplyRows + w;
  float v[kApplyRows / 4];
#pragma unroll
  for (int i = 0; i < kApplyRows / 4; ++i) {
    const int r = r0 + 4 * i;
    v[i] = r < a.B ? io<T>::ld(x + (size_t)r * a.d + col) : 0.f;
  }
#pragma unroll
  for (int i = 0; i < kApplyRows / 4; ++i) {
    const int r = r0 + 4 * i;
    if (r < a.B) io<T>::st(y + (size_t)r * a.d + col, (v[i] - mean) * rstd);
  }
}

// dx of the batch-statistics normalisation (training), or dx = dy * rstd (eval: the statistics are constants).
template <typename T>
__global__ __launch_bounds__(kStrip * kWaves) void bn1d_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                                    const float* __restrict__ mean_in,
                                                                    const float* __restrict__ rstd_in, T* __restrict__ dx,
                                                                    int B, int d, int training) {
#pragma clang fp reassociate(off) contract(off)
  __shared__ float s_part[kWaves][kStrip];
  __shared__ float s_res[kStrip];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = blockIdx.x * kStrip + lane;
  const bool cok = col < d;
  const float mean = cok ? mean_in[col] : 0.f, rstd = cok ? rstd_in[col] : 0.f;
  float m_dy = 0.f, m_dyx = 0.f;
  if (training) {                                // (uniform over the launch)
    float a0[4] = {0.f, 0.f, 0.f, 0.f}, a1[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r0 = w; r0 < B; r0 += 4 * kWaves) {
      float g[4], v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int r = r0 + u * kWaves;
        const bool ok = cok && r < B;
        g[u] = ok ? io<T>::ld(dy + (size_t)r * d + col) : 0.f;
        v[u] = ok ? io<T>::ld(x + (size_t)r * d + col) : mean;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a0[u] = a0[u] + g[u];
        a1[u] = a1[u] + g[u] * ((v[u] - mean) * rstd);
      }
    }
    const float invB = 1.f / (float)B;
    m_dy = strip_allsum((a0[0] + a0[1]) + (a0[2] + a0[3]), s_part, s_res) * invB;
    m_dyx = strip_allsum((a1[0] + a1[1]) + (a1[2] + a1[3]), s_part, s_res) * invB;
  }
  if (!cok) return;
  for (int r = w; r < B; r += kWaves) {
    const size_t i = (size_t)r * d + col;
    const float g = io<T>::ld(dy + i);
    const float xh = (io<T>::ld(x + i) - mean) * rstd;
    io<T>::st(dx + i, training ? rstd * ((g - m_dy) - xh * m_dyx) : g * rstd);
  }
}

}  // namespace

extern "C" int fv_bn1d_stats(const void* x, int dtype, float* table_row, int batch, int dim, fv_stream_t stream) {
  FV_CHECK(x && table_row, "bn1d_stats: null pointer");
  FV_CHECK(dtype == FV_F32 || dtype == FV_BF16, "bn1d_stats: features must be fp32 or bf16, got dtype %d", dtype);
  FV_CHECK(batch >= 1 && dim >= 1, "bn1d_stats: batch %d and dim %d must be positive", batch, dim);
  const dim3 grid(fv_cdiv(dim, kStrip)), block(kStrip * kWaves);
  hipStream_t st = (hipStream_t)stream;
  const bool reg = batch <= kWaves * kRegRows;
  if (dtype == FV_F32) {
    if (reg) hipLaunchKernelGGL((bn1d_stats_kernel<float, true>), grid, block, 0, st, (const float*)x, table_row, batch, dim);
    else hipLaunchKernelGGL((bn1d_stats_kernel<float, false>), grid, block, 0, st, (const float*)x, table_row, batch, dim);
  } else {
    if (reg) hipLaunchKernelGGL((bn1d_stats_kernel<bf16_t, true>), grid, block, 0, st, (const bf16_t*)x, table_row, batch, dim);
    else hipLaunchKernelGGL((bn1d_stats_kernel<bf16_t, false>), grid, block, 0, st, (const bf16_t*)x, table_row, batch, dim);
  }
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_bn1d_apply(const void* x, int dtype, const float* table, int world, float* running_mean,
                             float* running_var, int64_t* num_batches_tracked, void* xhat, float* mean_out,
                             float* rstd_out, int batch, int dim, float eps, float momentum, int training,
                             fv_stream_t stream) {
  FV_CHECK(x && xhat && mean_out && rstd_out, "bn1d_apply: null pointer");
  FV_CHECK(dtype == FV_F32 || dtype == FV_BF16, "bn1d_apply: features must be fp32 or bf16, got dtype %d", dtype);
  FV_CHECK(batch >= 1 && dim >= 1, "bn1d_apply: batch %d and dim %d must be positive", batch, dim);
  FV_CHECK((running_mean == nullptr) == (running_var == nullptr), "bn1d_apply: running_mean and running_var go together");
  if (training) {
    FV_CHECK(table && world >= 1, "bn1d_apply: training mode needs a statistics table of world >= 1 rows");
  } else {
    FV_CHECK(running_mean, "bn1d_apply: eval mode needs the running statistics");
  }
  FV_CHECK(momentum >= 0.f && momentum <= 1.f, "bn1d_apply: momentum %g outside [0, 1]", (double)momentum);
  BnApply a{};
  a.x = x; a.xhat = xhat; a.table = table; a.running_mean = running_mean; a.running_var = running_var;
  a.num_batches_tracked = reinterpret_cast<long long*>(num_batches_tracked);
  a.mean_out = mean_out; a.rstd_out = rstd_out;
  a.world = world; a.B = batch; a.d = dim; a.training = training ? 1 : 0; a.eps = eps; a.momentum = momentum;
  const dim3 grid(fv_cdiv(dim, kStrip), fv_cdiv(batch, kApplyRows));
  FV_CHECK(grid.y <= 65535u, "bn1d_apply: batch %d too large", batch);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == FV_F32) hipLaunchKernelGGL(bn1d_apply_kernel<float>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(bn1d_apply_kernel<bf16_t>, grid, dim3(256), 0, st, a);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_bn1d_bwd(const void* dy, const void* x, int dtype, const float* mean, const float* rstd, void* dx,
                           int batch, int dim, int training, fv_stream_t stream) {
  FV_CHECK(dy && x && mean && rstd && dx, "bn1d_bwd: null pointer");
  FV_CHECK(dtype == FV_F32 || dtype == FV_BF16, "bn1d_bwd: features must be fp32 or bf16, got dtype %d", dtype);
  FV_CHECK(batch >= 1 && dim >= 1, "bn1d_bwd: batch %d and dim %d must be positive", batch, dim);
  const dim3 grid(fv_cdiv(dim, kStrip)), block(kStrip * kWaves);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == FV_F32)
    hipLaunchKernelGGL(bn1d_bwd_kernel<float>, grid, block, 0, st, (const float*)dy, (const float*)x, mean, rstd, (float*)dx,
                       batch, dim, training ? 1 : 0);
  else
    hipLaunchKernelGGL(bn1d_bwd_kernel<bf16_t>, grid, block, 0, st, (const bf16_t*)dy, (const bf16_t*)x, mean, rstd,
                       (bf16_t*)dx, batch, dim, training ? 1 : 0);
  FV_LAUNCH_CHECK();
  return FV_OK;
}
