// LayerNorm over C where one side of the op is NCHW: the two kernels of the dense-prediction (detection / segmentation)
// recipes, forward and backward.
//
// * Feature tap (models/fastvim.py:682-690: ``outnorm_i(o.float())``, ``view(-1, H, W, C).permute(0, 3, 1, 2)
//   .contiguous()``): hidden states (B, H*W, C) token-major, bf16 / fp32  ->  affine LayerNorm over C  ->  fp32 (B, C, H, W).
// * LN2d (detection/vitdet/simple_fpn.py:15-32): channel LayerNorm of a contiguous (N, C, H, W) map, y in x's dtype.
//
// Every kernel stages ONE tile of P spatial positions x all C channels of one image in LDS as fp32.  The NCHW side of a
// tile is C plane segments of P contiguous elements; it moves between HBM and LDS in 16-byte groups cut at 16-byte
// boundaries of the tensor (tile_load / tile_store): a plane base that is not 16-byte aligned (odd H*W) costs the first
// and the last group of a segment, which go element by element, and nothing else.  The token-major side of the tap is a
// wave per token, 4 channels per lane per step, the row in registers.  Statistics are two exact passes in fp32 (mean,
// then the centred second moment) over the on-chip copy: the input is read from HBM once, the output written once.
//
// Weight / bias gradients: one partial row per workgroup, written (never accumulated), summed by fv_reduce_partials in
// fixed order -- no atomics, two runs are bit-identical.
#include <limits.h>

#include "rowwalk.h"

namespace {

constexpr int NT = 256;                      // threads per workgroup (4 waves)
constexpr int TAP_TP = 32;                   // tokens per tap tile: 8 per wave, all their loads in flight at once
constexpr int TAP_MAXC = 1024, LN2D_MAXC = 1024;
constexpr size_t LDS_TWO_WG = 80 * 1024;     // a tile up to this size leaves room for two workgroups per CU (160 KiB)
constexpr size_t LDS_LIMIT = 160 * 1024;

// LDS tile: row c holds the P positions of channel c (P a power of two), rotated by c >> SH.  SH = 0 (LN2d): lanes along
// the positions of one channel, or along channels at one position, both hit distinct banks.  SH = 2 (tap): a lane owns 4
// consecutive channels of one token, lane l's e-th access goes to bank (t + l) % 32.
template <int SH>
__device__ __forceinline__ int tidx(int c, int p, int P) { return c * P + ((p + (c >> SH)) & (P - 1)); }

// C plane segments [p0, p0 + n) of image `img_off` (element offset of the image in the tensor) -> LDS tile.
// Work item = (channel, 16-byte group of the tensor); a group that lies inside the segment is one vector load.
template <typename T, int SH>
__device__ __forceinline__ void tile_load(const T* __restrict__ g, size_t img_off, int HW, int p0, int n, int C, int P, float* s) {
  constexpr int V = 16 / sizeof(T);
  const int nq = P / V + 1;                  // groups a segment of P elements can touch when its base is unaligned
  for (int i = threadIdx.x; i < C * nq; i += NT) {
    const int c = i / nq, j = i - c * nq;
    const size_t g0 = img_off + (size_t)c * HW + p0;
    const int ts = j * V - (int)(g0 & (V - 1));            // position (relative to p0) of the group's first element
    if (ts >= n || ts + V <= 0) continue;
    if (ts >= 0 && ts + V <= n) {
      float v[V];
      VecIO<T, V>::load(g + g0 + ts, v);
#pragma unroll
      for (int e = 0; e < V; ++e) s[tidx<SH>(c, ts + e, P)] = v[e];
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const int t = ts + e;
        if (t >= 0 && t < n) s[tidx<SH>(c, t, P)] = io<T>::ld(g + g0 + t);
      }
    }
  }
}

template <typename T, int SH>
__device__ __forceinline__ void tile_store(T* __restrict__ g, size_t img_off, int HW, int p0, int n, int C, int P, const float* s) {
  constexpr int V = 16 / sizeof(T);
  const int nq = P / V + 1;
  for (int i = threadIdx.x; i < C * nq; i += NT) {
    const int c = i / nq, j = i - c * nq;
    const size_t g0 = img_off + (size_t)c * HW + p0;
    const int ts = j * V - (int)(g0 & (V - 1));
    if (ts >= n || ts + V <= 0) continue;
    if (ts >= 0 && ts + V <= n) {
      float v[V];
#pragma unroll
      for (int e = 0; e < V; ++e) v[e] = s[tidx<SH>(c, ts + e, P)];
      VecIO<T, V>::store(g + g0 + ts, v);
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const int t = ts + e;
        if (t >= 0 && t < n) io<T>::st(g + g0 + t, s[tidx<SH>(c, t, P)]);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ feature tap
struct TapParams {
  const void* x;
  const float *w, *b, *dy, *mean_in, *rstd_in;
  float *y, *mean, *rstd, *pw, *pb;
  void* dx;
  int B, L, C, tiles;
  float eps;
};

// wave wv owns tokens u * 4 + wv of the tile (u = 0 .. 7): the rows of all of them are loaded before the first wait
template <typename T, int MAXK>
__device__ __forceinline__ void tap_load_rows(const T* x, int n, int C, int wv, int lane, float (&v)[TAP_TP / 4][MAXK][4]) {
#pragma unroll
  for (int u = 0; u < TAP_TP / 4; ++u) {
    const int t = u * 4 + wv;
#pragma unroll
    for (int k = 0; k < MAXK; ++k) {
      const int c = (k * 64 + lane) * 4;
      if (t < n && c < C) {
        VecIO<T, 4>::load(x + (size_t)t * C + c, v[u][k]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[u][k][e] = 0.f;
      }
    }
  }
}

template <typename T, int MAXK>
__global__ __launch_bounds__(NT) void tap_fwd_kernel(TapParams p) {
  extern __shared__ __attribute__((aligned(16))) float s_tile[];
  constexpr int RU = TAP_TP / 4;
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.x / p.tiles, l0 = (blockIdx.x - b * p.tiles) * TAP_TP;
  const int n = min(TAP_TP, p.L - l0), C = p.C;
  const size_t row0 = (size_t)b * p.L + l0;
  float v[RU][MAXK][4];
  tap_load_rows<T, MAXK>((const T*)p.x + row0 * C, n, C, wv, lane, v);
  float w[MAXK][4], bb[MAXK][4];
#pragma unroll
  for (int k = 0; k < MAXK; ++k) {
    const int c = (k * 64 + lane) * 4;
    if (c < C) {
      VecIO<float, 4>::load(p.w + c, w[k]);
      VecIO<float, 4>::load(p.b + c, bb[k]);
    }
  }
  const float inv_c = 1.f / (float)C;
#pragma unroll
  for (int u = 0; u < RU; ++u) {
    const int t = u * 4 + wv;                  // wave-uniform
    if (t >= n) break;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < MAXK; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) s += v[u][k][e];           // lanes past C hold zeros
    const float mu = wave_sum(s) * inv_c;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < MAXK; ++k) {
      if ((k * 64 + lane) * 4 < C) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = v[u][k][e] - mu;
          q = fmaf(d, d, q);
        }
      }
    }
    const float rstd = rsqrtf(wave_sum(q) * inv_c + p.eps);
    if (lane == 0) {
      p.mean[row0 + t] = mu;
      p.rstd[row0 + t] = rstd;
    }
#pragma unroll
    for (int k = 0; k < MAXK; ++k) {
      const int c = (k * 64 + lane) * 4;
      if (c < C) {
#pragma unroll
        for (int e = 0; e < 4; ++e) s_tile[tidx<2>(c + e, t, TAP_TP)] = (v[u][k][e] - mu) * rstd * w[k][e] + bb[k][e];
      }
    }
  }
  __syncthreads();
  tile_store<float, 2>(p.y, (size_t)b * C * p.L, p.L, l0, n, C, TAP_TP, s_tile);
}

// d x = rstd * (dxhat - mean(dxhat) - xhat * mean(dxhat * xhat)), dxhat = dy * w; per-workgroup partial rows of
// d w = sum dy * xhat and d b = sum dy
template <typename T, int MAXK>
__global__ __launch_bounds__(NT) void tap_bwd_kernel(TapParams p) {
  extern __shared__ __attribute__((aligned(16))) float s_tile[];
  constexpr int RU = TAP_TP / 4;
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.x / p.tiles, l0 = (blockIdx.x - b * p.tiles) * TAP_TP;
  const int n = min(TAP_TP, p.L - l0), C = p.C;
  const size_t row0 = (size_t)b * p.L + l0;
  float xr[RU][MAXK][4];
  tap_load_rows<T, MAXK>((const T*)p.x + row0 * C, n, C, wv, lane, xr);      // in flight while the dy tile is staged
  tile_load<float, 2>(p.dy, (size_t)b * C * p.L, p.L, l0, n, C, TAP_TP, s_tile);
  float w[MAXK][4], aw[MAXK][4], ab[MAXK][4];
#pragma unroll
  for (int k = 0; k < MAXK; ++k) {
    const int c = (k * 64 + lane) * 4;
    if (c < C) VecIO<float, 4>::load(p.w + c, w[k]);
#pragma unroll
    for (int e = 0; e < 4; ++e) aw[k][e] = ab[k][e] = 0.f;
  }
  __syncthreads();
  const float inv_c = 1.f / (float)C;
  T* dx = (T*)p.dx + row0 * C;
#pragma unroll
  for (int u = 0; u < RU; ++u) {
    const int t = u * 4 + wv;
    if (t >= n) break;
    const float mu = p.mean_in[row0 + t], rstd = p.rstd_in[row0 + t];
    float xh[MAXK][4], g[MAXK][4];
    float c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int k = 0; k < MAXK; ++k) {
      const int c = (k * 64 + lane) * 4;
      if (c < C) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = s_tile[tidx<2>(c + e, t, TAP_TP)];
          xh[k][e] = (xr[u][k][e] - mu) * rstd;
          g[k][e] = d * w[k][e];
          aw[k][e] = fmaf(d, xh[k][e], aw[k][e]);
          ab[k][e] += d;
          c1 += g[k][e];
          c2 = fmaf(g[k][e], xh[k][e], c2);
        }
      }
    }
    c1 = wave_sum(c1) * inv_c;
    c2 = wave_sum(c2) * inv_c;
#pragma unroll
    for (int k = 0; k < MAXK; ++k) {
      const int c = (k * 64 + lane) * 4;
      if (c < C) {
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = rstd * (g[k][e] - c1 - xh[k][e] * c2);
        VecIO<T, 4>::store(dx + (size_t)t * C + c, o);
      }
    }
  }
  // the 4 waves' accumulators through LDS (4 * C <= 32 * C floats of the tile), fixed order -> one partial row
  for (int pass = 0; pass < 2; ++pass) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < MAXK; ++k) {
      const int c = (k * 64 + lane) * 4;
      if (c < C)
#pragma unroll
        for (int e = 0; e < 4; ++e) s_tile[wv * C + c + e] = pass ? ab[k][e] : aw[k][e];
    }
    __syncthreads();
    float* dst = (pass ? p.pb : p.pw) + (size_t)blockIdx.x * C;
    for (int c = threadIdx.x; c < C; c += NT)
      dst[c] = (s_tile[c] + s_tile[C + c]) + (s_tile[2 * C + c] + s_tile[3 * C + c]);
  }
}

// ------------------------------------------------------------------------------------------------ LN2d
struct Ln2dParams {
  const void *x, *dy;
  const float *w, *b, *mean_in, *rstd_in;
  void *y, *dx;
  float *mean, *rstd, *pw, *pb;
  int C, HW, P, logP, tiles;
  float eps;
};

// Thread = (position pp of the tile, channel slice q of S = 256 / P): lanes run along the contiguous spatial index, the
// sums over C walk the tile's rows; the S slice sums of a position meet in LDS and are added in slice order.
template <typename T>
__global__ __launch_bounds__(NT) void ln2d_fwd_kernel(Ln2dParams p) {
  extern __shared__ __attribute__((aligned(16))) float s_tile[];
  const int C = p.C, P = p.P, S = NT >> p.logP;
  float* red = s_tile + (size_t)C * P;         // NT floats
  const int img = blockIdx.x / p.tiles, p0 = (blockIdx.x - img * p.tiles) * P;
  const int n = min(P, p.HW - p0);
  const size_t img_off = (size_t)img * C * p.HW;
  tile_load<T, 0>((const T*)p.x, img_off, p.HW, p0, n, C, P, s_tile);
  __syncthreads();
  const int pp = threadIdx.x & (P - 1), q = threadIdx.x >> p.logP;
  const float inv_c = 1.f / (float)C;
  // positions past n (the last tile of an image) run on whatever the tile holds there; nothing of them is stored
  float a = 0.f;
  for (int c = q; c < C; c += S) a += s_tile[tidx<0>(c, pp, P)];
  red[threadIdx.x] = a;
  __syncthreads();
  float mu = 0.f;
  for (int j = 0; j < S; ++j) mu += red[j * P + pp];
  mu *= inv_c;
  __syncthreads();
  a = 0.f;
  for (int c = q; c < C; c += S) {
    const float d = s_tile[tidx<0>(c, pp, P)] - mu;
    a = fmaf(d, d, a);
  }
  red[threadIdx.x] = a;
  __syncthreads();
  float var = 0.f;
  for (int j = 0; j < S; ++j) var += red[j * P + pp];
  const float rstd = rsqrtf(var * inv_c + p.eps);
  if (q == 0 && pp < n) {
    p.mean[(size_t)img * p.HW + p0 + pp] = mu;
    p.rstd[(size_t)img * p.HW + p0 + pp] = rstd;
  }
  for (int c = q; c < C; c += S) {
    const int i = tidx<0>(c, pp, P);
    s_tile[i] = (s_tile[i] - mu) * rstd * p.w[c] + p.b[c];
  }
  __syncthreads();
  tile_store<T, 0>((T*)p.y, img_off, p.HW, p0, n, C, P, s_tile);
}

template <typename T>
__global__ __launch_bounds__(NT) void ln2d_bwd_kernel(Ln2dParams p) {
  extern __shared__ __attribute__((aligned(16))) float s_tile[];
  const int C = p.C, P = p.P, S = NT >> p.logP;
  float* sx = s_tile;                          // x, then xhat
  float* sd = s_tile + (size_t)C * P;          // dy, then dx
  float* red = sd + (size_t)C * P;             // 2 * NT floats
  const int img = blockIdx.x / p.tiles, p0 = (blockIdx.x - img * p.tiles) * P;
  const int n = min(P, p.HW - p0);
  const size_t img_off = (size_t)img * C * p.HW;
  tile_load<T, 0>((const T*)p.x, img_off, p.HW, p0, n, C, P, sx);
  tile_load<T, 0>((const T*)p.dy, img_off, p.HW, p0, n, C, P, sd);
  const int pp = threadIdx.x & (P - 1), q = threadIdx.x >> p.logP;
  const bool live = pp < n;
  const float mu = live ? p.mean_in[(size_t)img * p.HW + p0 + pp] : 0.f;
  const float rstd = live ? p.rstd_in[(size_t)img * p.HW + p0 + pp] : 0.f;
  __syncthreads();
  const float inv_c = 1.f / (float)C;
  float c1 = 0.f, c2 = 0.f;
  for (int c = q; c < C; c += S) {
    const int i = tidx<0>(c, pp, P);
    const float xh = (sx[i] - mu) * rstd;
    const float g = sd[i] * p.w[c];
    sx[i] = xh;
    c1 += g;
    c2 = fmaf(g, xh, c2);
  }
  red[threadIdx.x] = c1;
  red[NT + threadIdx.x] = c2;
  __syncthreads();
  c1 = c2 = 0.f;
  for (int j = 0; j < S; ++j) {
    c1 += red[j * P + pp];
    c2 += red[NT + j * P + pp];
  }
  c1 *= inv_c;
  c2 *= inv_c;
  // this workgroup's partial row of d w / d b: a thread per channel, the tile's n positions in order
  for (int c = threadIdx.x; c < C; c += NT) {
    float aw = 0.f, ab = 0.f;
    for (int t = 0; t < n; ++t) {
      const int i = tidx<0>(c, t, P);
      const float d = sd[i];
      aw = fmaf(d, sx[i], aw);
      ab += d;
    }
    p.pw[(size_t)blockIdx.x * C + c] = aw;
    p.pb[(size_t)blockIdx.x * C + c] = ab;
  }
  __syncthreads();
  for (int c = q; c < C; c += S) {
    const int i = tidx<0>(c, pp, P);
    sd[i] = rstd * (sd[i] * p.w[c] - c1 - sx[i] * c2);
  }
  __syncthreads();
  tile_store<T, 0>((T*)p.dx, img_off, p.HW, p0, n, C, P, sd);
}

// positions per LN2d tile: 64 (256-byte fp32 segments) while `ntiles` tiles of C x P fp32 leave room for two workgroups
// per CU, never below 16; an image smaller than half a tile takes the smaller tile.  C <= 1024 keeps 2 x C x 16 x 4 B
// (128 KiB) plus the reduction scratch inside the 160 KiB of a CU.
int ln2d_positions(int C, int HW, int ntiles) {
  int P = 64;
  while (P > 16 && ((size_t)ntiles * C * P * sizeof(float) > LDS_TWO_WG || P / 2 >= HW)) P >>= 1;
  return P;
}
int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <typename K>
void allow_big_lds(K kernel, FvOncePerDevice& done) {
  if (done.first()) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_LIMIT);
}

template <typename T, int MAXK>
void tap_launch(bool bwd, const TapParams& p, int blocks, size_t lds, hipStream_t st) {
  static FvOncePerDevice done_f, done_b;
  if (bwd) {
    allow_big_lds(tap_bwd_kernel<T, MAXK>, done_b);
    hipLaunchKernelGGL((tap_bwd_kernel<T, MAXK>), dim3(blocks), dim3(NT), lds, st, p);
  } else {
    allow_big_lds(tap_fwd_kernel<T, MAXK>, done_f);
    hipLaunchKernelGGL((tap_fwd_kernel<T, MAXK>), dim3(blocks), dim3(NT), lds, st, p);
  }
}
template <typename T>
void tap_dispatch(bool bwd, const TapParams& p, int blocks, hipStream_t st) {
  const size_t lds = (size_t)p.C * TAP_TP * sizeof(float);
  if (p.C <= 256) tap_launch<T, 1>(bwd, p, blocks, lds, st);
  else if (p.C <= 512) tap_launch<T, 2>(bwd, p, blocks, lds, st);
  else if (p.C <= 768) tap_launch<T, 3>(bwd, p, blocks, lds, st);
  else tap_launch<T, 4>(bwd, p, blocks, lds, st);
}

template <typename T>
void ln2d_launch(bool bwd, const Ln2dParams& p, int blocks, hipStream_t st) {
  static FvOncePerDevice done_f, done_b;
  const size_t lds = ((size_t)(bwd ? 2 : 1) * p.C * p.P + (bwd ? 2 : 1) * NT) * sizeof(float);
  if (bwd) {
    allow_big_lds(ln2d_bwd_kernel<T>, done_b);
    hipLaunchKernelGGL(ln2d_bwd_kernel<T>, dim3(blocks), dim3(NT), lds, st, p);
  } else {
    allow_big_lds(ln2d_fwd_kernel<T>, done_f);
    hipLaunchKernelGGL(ln2d_fwd_kernel<T>, dim3(blocks), dim3(NT), lds, st, p);
  }
}

}  // namespace

#define FV_TAP_SHAPE_CHECKS(what)                                                                                        \
  FV_CHECK(B > 0 && L > 0, what ": empty input (B = %d, H*W = %d)", B, L);                                               \
  FV_CHECK(C >= 4 && C % 4 == 0 && C <= TAP_MAXC, what ": C = %d must be a multiple of 4 in [4, %d]", C, TAP_MAXC);      \
  FV_CHECK((long)B * ((L + TAP_TP - 1) / TAP_TP) <= INT_MAX, what ": B = %d x H*W = %d is too many tiles", B, L);        \
  FV_CHECK(x_dtype == FV_F32 || x_dtype == FV_BF16, what ": dtype code %d must be fp32 or bf16", x_dtype)

extern "C" int fv_tap_ln_blocks(int B, int L) {
  if (B <= 0 || L <= 0) return 0;
  const long blocks = (long)B * ((L + TAP_TP - 1) / TAP_TP);
  return blocks <= INT_MAX ? (int)blocks : 0;
}

extern "C" int fv_tap_ln_fwd(const void* x, int x_dtype, const float* weight, const float* bias, float* y, float* mean,
                             float* rstd, int B, int L, int C, float eps, fv_stream_t stream) {
  FV_TAP_SHAPE_CHECKS("tap_ln_fwd");
  FV_CHECK(x && weight && bias && y && mean && rstd, "tap_ln_fwd: null pointer");
  FV_CHECK(aligned16(x) && aligned16(y) && aligned16(weight) && aligned16(bias), "tap_ln_fwd: x, y, weight and bias must be 16-byte aligned");
  TapParams p{};
  p.x = x; p.w = weight; p.b = bias; p.y = y; p.mean = mean; p.rstd = rstd;
  p.B = B; p.L = L; p.C = C; p.tiles = (L + TAP_TP - 1) / TAP_TP; p.eps = eps;
  if (x_dtype == FV_F32) tap_dispatch<float>(false, p, B * p.tiles, (hipStream_t)stream);
  else tap_dispatch<bf16_t>(false, p, B * p.tiles, (hipStream_t)stream);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_tap_ln_bwd(const float* dy, const void* x, int x_dtype, const float* weight, const float* mean,
                             const float* rstd, void* dx, float* partial_dw, float* partial_db, int B, int L, int C,
                             fv_stream_t stream) {
  FV_TAP_SHAPE_CHECKS("tap_ln_bwd");
  FV_CHECK(dy && x && weight && mean && rstd && dx && partial_dw && partial_db, "tap_ln_bwd: null pointer");
  FV_CHECK(aligned16(dy) && aligned16(x) && aligned16(dx) && aligned16(weight), "tap_ln_bwd: dy, x, dx and weight must be 16-byte aligned");
  TapParams p{};
  p.dy = dy; p.x = x; p.w = weight; p.mean_in = mean; p.rstd_in = rstd; p.dx = dx; p.pw = partial_dw; p.pb = partial_db;
  p.B = B; p.L = L; p.C = C; p.tiles = (L + TAP_TP - 1) / TAP_TP;
  if (x_dtype == FV_F32) tap_dispatch<float>(true, p, B * p.tiles, (hipStream_t)stream);
  else tap_dispatch<bf16_t>(true, p, B * p.tiles, (hipStream_t)stream);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

#define FV_LN2D_SHAPE_CHECKS(what)                                                                                       \
  FV_CHECK(N > 0 && HW > 0, what ": empty input (N = %d, H*W = %d)", N, HW);                                             \
  FV_CHECK(C >= 1 && C <= LN2D_MAXC, what ": C = %d must be in [1, %d]", C, LN2D_MAXC);                                  \
  FV_CHECK(dtype == FV_F32 || dtype == FV_BF16, what ": dtype code %d must be fp32 or bf16", dtype)

static long ln2d_block_count(int N, int C, int HW, int ntiles, int* P_out) {
  const int P = ln2d_positions(C, HW, ntiles);
  if (P_out) *P_out = P;
  return (long)N * ((HW + P - 1) / P);
}

extern "C" int fv_ln2d_blocks(int N, int C, int HW) {
  if (N <= 0 || HW <= 0 || C < 1 || C > LN2D_MAXC) return 0;
  const long blocks = ln2d_block_count(N, C, HW, 2, nullptr);
  return blocks <= INT_MAX ? (int)blocks : 0;
}

extern "C" int fv_ln2d_fwd(const void* x, int dtype, const float* weight, const float* bias, void* y, float* mean,
                           float* rstd, int N, int C, int HW, float eps, fv_stream_t stream) {
  FV_LN2D_SHAPE_CHECKS("ln2d_fwd");
  FV_CHECK(x && weight && bias && y && mean && rstd, "ln2d_fwd: null pointer");
  FV_CHECK(aligned16(x) && aligned16(y), "ln2d_fwd: x and y must be 16-byte aligned");
  Ln2dParams p{};
  const long blocks = ln2d_block_count(N, C, HW, 1, &p.P);
  FV_CHECK(blocks <= INT_MAX, "ln2d_fwd: N = %d x H*W = %d is too many tiles", N, HW);
  p.x = x; p.w = weight; p.b = bias; p.y = y; p.mean = mean; p.rstd = rstd;
  p.C = C; p.HW = HW; p.logP = ilog2(p.P); p.tiles = (HW + p.P - 1) / p.P; p.eps = eps;
  if (dtype == FV_F32) ln2d_launch<float>(false, p, (int)blocks, (hipStream_t)stream);
  else ln2d_launch<bf16_t>(false, p, (int)blocks, (hipStream_t)stream);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_ln2d_bwd(const void* dy, const void* x, int dtype, const float* weight, const float* mean,
                           const float* rstd, void* dx, float* partial_dw, float* partial_db, int N, int C, int HW,
                           fv_stream_t stream) {
  FV_LN2D_SHAPE_CHECKS("ln2d_bwd");
  FV_CHECK(dy && x && weight && mean && rstd && dx && partial_dw && partial_db, "ln2d_bwd: null pointer");
  FV_CHECK(aligned16(dy) && aligned16(x) && aligned16(dx), "ln2d_bwd: dy, x and dx must be 16-byte aligned");
  Ln2dParams p{};
  const long blocks = ln2d_block_count(N, C, HW, 2, &p.P);
  FV_CHECK(blocks <= INT_MAX, "ln2d_bwd: N = %d x H*W = %d is too many tiles", N, HW);
  p.dy = dy; p.x = x; p.w = weight; p.mean_in = mean; p.rstd_in = rstd; p.dx = dx; p.pw = partial_dw; p.pb = partial_db;
  p.C = C; p.HW = HW; p.logP = ilog2(p.P); p.tiles = (HW + p.P - 1) / p.P;
  if (dtype == FV_F32) ln2d_launch<float>(true, p, (int)blocks, (hipStream_t)stream);
  else ln2d_launch<bf16_t>(true, p, (int)blocks, (hipStream_t)stream);
  FV_LAUNCH_CHECK();
  return FV_OK;
}
