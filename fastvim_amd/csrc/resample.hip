// hipcc-flags: -fno-fast-math -ffp-contract=off
// Device-side geometry of the uint8 loaders: PIL's 8-bit bicubic resize (ImagingResample: horizontal pass, uint8
// intermediate, vertical pass, integer coefficients of 22 fraction bits), a crop window of the result and a horizontal
// flip, bit for bit (include/fastvim_hip.h at fv_resample_coeffs; restated in numpy at tests/resample_ref.py).
//
//   resample_coeffs_kernel   one workgroup per (sample, axis), one thread per output of the window: the filter bounds
//                            (lo, cnt) and the cnt integer coefficients, computed in fp64 exactly as PIL's
//                            precompute_coeffs / normalize_coeffs_8bpc do -- this file is built WITHOUT fast-math and
//                            with contraction off, so every operation below is the IEEE one, in the order written.
//                            Written as c[k][i]: lanes that own neighbouring outputs read neighbouring words.
//   resample_u8_kernel       a workgroup owns FV_RESAMPLE_BAND output rows x up to 256 output columns of one sample.  It
//                            walks the band in sub-bands: as many output rows as have their source rows in the LDS tile
//                            (at least one: 65 taps x 256 columns x 3 channels = 49,920 B; with the band's y bounds and
//                            y coefficients in front of it 54,208 B, three workgroups per CU).
//                            Horizontal pass: a thread per (four source rows, output column), three channels, loads
//                            that are legal at any byte address (rows of 3 w_src bytes start anywhere), uint8 into the tile,
//                            which is PLANAR (channel, row, column) so that the vertical pass reads four neighbouring
//                            columns of a channel as one dword.  Vertical pass: a thread per (output row, channel, four
//                            columns); the flip mirrors the store (a byte-reversed dword at the mirrored address).
//
// Integer arithmetic of a pass: clip((2^21 + sum_k src[lo + k] c_k) >> 22, 0, 255), int32, arithmetic shift.
// A plan row outside the served range never reaches a load: the coefficient launch gives it cnt = 0 everywhere.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int RS_TAPS = FV_RESAMPLE_MAX_TAPS;
constexpr int RS_PLAN = FV_RESAMPLE_PLAN_INTS;
constexpr int RS_BAND = FV_RESAMPLE_BAND;
constexpr int RS_TW = 256;                          // output columns per workgroup
constexpr int RS_THREADS = 256;
constexpr int RS_LDS = 3 * RS_TAPS * RS_TW;         // 49,920 B: every tap row of one output row at the full tile width
constexpr int RS_HDR = (2 + RS_TAPS) * RS_BAND * 4; // 4,288 B in front of the tile: the band's y bounds and y coefficients
constexpr int RS_PRECISION_BITS = 22;

__host__ __device__ inline bool launch_ok(int batch, int s_h, int s_w) {
  return batch >= 1 && batch <= 4096 && s_h >= 8 && s_h <= 1024 && s_w >= 8 && s_w <= 1024;
}

__host__ __device__ inline bool sample_ok(int s_h, int s_w, int h_src, int w_src, int o_h, int o_w, int win_y, int win_x) {
  if (h_src < 1 || h_src > 16384 || w_src < 1 || w_src > 16384) return false;
  if (o_h < 1 || o_h > 65536 || o_w < 1 || o_w > 65536) return false;
  if (win_y < 0 || win_x < 0 || win_y > o_h - s_h || win_x > o_w - s_w) return false;
  return h_src <= 16 * o_h && w_src <= 16 * o_w;      // scale <= 16: at most 65 taps
}

// words of one sample's workspace: x axis, then y axis
__host__ __device__ inline long sample_ws_ints(int s_h, int s_w) { return (long)(s_h + s_w) * (2 + RS_TAPS); }

struct PlanRow {
  long long off;
  int h_src, w_src, o_h, o_w, win_y, win_x, flip;
};

__device__ __forceinline__ PlanRow read_plan(const int* __restrict__ plan, int b) {
  const int* p = plan + (size_t)b * RS_PLAN;
  PlanRow r;
  r.off = (long long)(((unsigned long long)(unsigned)p[1] << 32) | (unsigned long long)(unsigned)p[0]);
  r.h_src = p[2]; r.w_src = p[3]; r.o_h = p[4]; r.o_w = p[5]; r.win_y = p[6]; r.win_x = p[7]; r.flip = p[8];
  return r;
}

// PIL's bicubic_filter, a = -0.5
__device__ __forceinline__ double bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

__global__ __launch_bounds__(RS_THREADS) void resample_coeffs_kernel(const int* __restrict__ plan, long long pool_bytes,
                                                                     int* __restrict__ ws, int s_h, int s_w) {
  const int axis = blockIdx.x, b = blockIdx.y;
  const PlanRow P = read_plan(plan, b);
  bool valid = sample_ok(s_h, s_w, P.h_src, P.w_src, P.o_h, P.o_w, P.win_y, P.win_x);
  valid = valid && P.off >= 0 && P.off <= pool_bytes && (long long)P.h_src * P.w_src * 3 <= pool_bytes - P.off;
  const int n = axis == 0 ? P.w_src : P.h_src, m = axis == 0 ? P.o_w : P.o_h;
  const int win = axis == 0 ? P.win_x : P.win_y, S = axis == 0 ? s_w : s_h;
  int* bounds = ws + (size_t)b * sample_ws_ints(s_h, s_w) + (axis == 0 ? 0 : (size_t)s_w * (2 + RS_TAPS));
  int* coef = bounds + 2 * S;
  for (int i = threadIdx.x; i < S; i += RS_THREADS) {
    int lo = 0, cnt = 0;
    if (valid) {
      const double scale = (double)n / (double)m;
      const double fs = scale < 1.0 ? 1.0 : scale;
      const double support = 2.0 * fs;
      const double ss = 1.0 / fs;
      const double center = ((win + i) + 0.5) * scale;
      lo = (int)(center - support + 0.5);
      if (lo < 0) lo = 0;
      int hi = (int)(center + support + 0.5);
      if (hi > n) hi = n;
      cnt = hi - lo;
      if (cnt > RS_TAPS) cnt = RS_TAPS;       // (cannot happen for scale <= 16; the workspace has RS_TAPS rows)
      if (cnt < 0) cnt = 0;
      double ww = 0.0;
      for (int k = 0; k < cnt; ++k) ww += bicubic(((k + lo) - center + 0.5) * ss);
      for (int k = 0; k < cnt; ++k) {
        double w = bicubic(((k + lo) - center + 0.5) * ss);
        if (ww != 0.0) w /= ww;
        const double q = w * (double)(1 << RS_PRECISION_BITS);
        coef[(size_t)k * S + i] = w < 0 ? (int)(-0.5 + q) : (int)(0.5 + q);
      }
    }
    bounds[i] = lo;
    bounds[S + i] = cnt;
  }
}

// four bytes at any address: the compiler picks a load that is legal for alignment 1 (one dword load on gfx950)
__device__ __forceinline__ uint32_t ld32_unaligned(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> RS_PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ __launch_bounds__(RS_THREADS) void resample_u8_kernel(const uint8_t* __restrict__ pool,
                                                                 const int* __restrict__ plan, const int* __restrict__ ws,
                                                                 uint8_t* __restrict__ out, long long pool_bytes, int s_h,
                                                                 int s_w, int pitch, int rows_cap, int out_vec) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  int* s_lo = reinterpret_cast<int*>(smem);     // [RS_BAND] first source row of the band's output rows
  int* s_cnt = s_lo + RS_BAND;                  // [RS_BAND] their tap counts
  int* s_cy = s_cnt + RS_BAND;                  // [RS_TAPS][RS_BAND] their coefficients
  uint8_t* tile = smem + RS_HDR;                // (3, rows_cap, pitch)
  const int b = blockIdx.z, tid = threadIdx.x;
  const int x0 = blockIdx.x * RS_TW, tw = min(RS_TW, s_w - x0);
  const int y_begin = blockIdx.y * RS_BAND, y_end = min(y_begin + RS_BAND, s_h);
  const PlanRow P = read_plan(plan, b);
  // the coefficient launch's own check: a workspace that was not made for this plan must not steer a load out of the pool
  const bool valid = sample_ok(s_h, s_w, P.h_src, P.w_src, P.o_h, P.o_w, P.win_y, P.win_x) && P.off >= 0 &&
                     P.off <= pool_bytes && (long long)P.h_src * P.w_src * 3 <= pool_bytes - P.off;
  const int* bx = ws + (size_t)b * sample_ws_ints(s_h, s_w);
  const int* cx = bx + 2 * s_w;
  const int* by = bx + (size_t)s_w * (2 + RS_TAPS);
  const int* cy = by + 2 * s_h;
  const uint8_t* src = pool + P.off;
  const int plane = rows_cap * pitch, q = pitch >> 2;
  const size_t row_bytes = (size_t)P.w_src * 3;

  // the band's y tables once, so that neither the sub-band search nor the vertical taps wait for global memory
  const int nb = y_end - y_begin;
  if (tid < nb) {
    s_lo[tid] = by[y_begin + tid];
    s_cnt[tid] = min(max(by[s_h + y_begin + tid], 0), RS_TAPS);
  }
  __syncthreads();
  for (int idx = tid; idx < RS_TAPS * RS_BAND; idx += RS_THREADS) {
    const int k = idx / RS_BAND, j = idx % RS_BAND;
    if (j < nb && k < s_cnt[j]) s_cy[idx] = cy[(size_t)k * s_h + y_begin + j];
  }
  __syncthreads();

  for (int y = y_begin; y < y_end;) {
    // the sub-band: output rows y .. y + n - 1 whose source rows row0 .. row1 - 1 fit the tile (lo and hi do not decrease)
    const int yb = y - y_begin;
    const int row0 = s_lo[yb];
    int row1 = row0 + s_cnt[yb], n = 1;
    while (y + n < y_end) {
      const int e = s_lo[yb + n] + s_cnt[yb + n];
      if (e - row0 > rows_cap) break;
      row1 = max(row1, e);
      ++n;
    }
    const int nrows = min(row1 - row0, rows_cap);

    // horizontal pass: source rows row0 .. row1 - 1, output columns x0 .. x0 + tw - 1; a thread owns one column of FOUR
    // rows, so a coefficient is loaded once per four rows and twelve sums are in flight.  A tap is one 4-byte load at its
    // (arbitrarily aligned) pixel -- R, G, B and the first byte of the next tap -- except the last tap, which is three
    // byte loads: nothing past the last pixel of a row is ever read.
    const bool rows_ok = valid && row0 >= 0 && row0 + nrows <= P.h_src;
    const int groups = (nrows + 3) >> 2;
    for (int idx = tid; idx < groups * tw; idx += RS_THREADS) {
      const int g = idx / tw, xl = idx - g * tw, i = x0 + xl, r0 = 4 * g;
      const int lo = bx[i];
      int cnt = min(bx[s_w + i], RS_TAPS);
      if (!rows_ok || lo < 0) cnt = 0;
      cnt = min(cnt, P.w_src - lo);
      const uint8_t* s[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] = src + (size_t)(row0 + min(r0 + j, nrows - 1)) * row_bytes + (size_t)lo * 3;
      const int* c = cx + i;
      int acc[4][3];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 1 << (RS_PRECISION_BITS - 1);
      for (int k = 0; k < cnt - 1; ++k) {
        const int w = c[(size_t)k * s_w];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t v = ld32_unaligned(s[j] + 3 * k);
          acc[j][0] += (int)(v & 0xffu) * w;
          acc[j][1] += (int)((v >> 8) & 0xffu) * w;
          acc[j][2] += (int)((v >> 16) & 0xffu) * w;
        }
      }
      if (cnt > 0) {
        const int k = cnt - 1, w = c[(size_t)k * s_w];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[j][0] += (int)s[j][3 * k] * w;
          acc[j][1] += (int)s[j][3 * k + 1] * w;
          acc[j][2] += (int)s[j][3 * k + 2] * w;
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (r0 + j < nrows) {
          uint8_t* t = tile + (r0 + j) * pitch + xl;
          t[0] = (uint8_t)clip8(acc[j][0]);
          t[plane] = (uint8_t)clip8(acc[j][1]);
          t[2 * plane] = (uint8_t)clip8(acc[j][2]);
        }
      }
    }
    __syncthreads();

    // vertical pass: a thread per (output row, channel, four columns)
    for (int idx = tid; idx < n * 3 * q; idx += RS_THREADS) {
      const int g = idx % q, t = idx / q;
      const int c = t % 3, yl = yb + t / 3, yo = y_begin + yl;
      const int xl = 4 * g;
      if (xl >= tw) continue;
      const int lo = s_lo[yl] - row0;
      const int cnt = lo < 0 ? 0 : min(s_cnt[yl], nrows - lo);
      const uint32_t* p = reinterpret_cast<const uint32_t*>(tile + c * plane + lo * pitch + xl);
      const int* cf = s_cy + yl;
      int acc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = 1 << (RS_PRECISION_BITS - 1);
      for (int k = 0; k < cnt; ++k) {
        const int w = cf[k * RS_BAND];
        const uint32_t v = p[k * q];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += (int)((v >> (8 * j)) & 0xffu) * w;
      }
      uint8_t* o = out + (((size_t)b * 3 + c) * s_h + yo) * s_w;
      const int x = x0 + xl, nv = min(4, tw - xl);
      const uint32_t v0 = clip8(acc[0]), v1 = clip8(acc[1]), v2 = clip8(acc[2]), v3 = clip8(acc[3]);
      if (out_vec && nv == 4) {               // s_w % 4 == 0 and out 4-byte aligned: x and s_w - 4 - x are multiples of 4
        if (P.flip) *reinterpret_cast<uint32_t*>(o + (s_w - 4 - x)) = v3 | (v2 << 8) | (v1 << 16) | (v0 << 24);
        else *reinterpret_cast<uint32_t*>(o + x) = v0 | (v1 << 8) | (v2 << 16) | (v3 << 24);
      } else {
        const uint32_t pk = v0 | (v1 << 8) | (v2 << 16) | (v3 << 24);
        for (int j = 0; j < nv; ++j) {
          const int xd = P.flip ? s_w - 1 - (x + j) : x + j;
          o[xd] = (uint8_t)(pk >> (8 * j));
        }
      }
    }
    __syncthreads();
    y += n;
  }
}

}  // namespace

extern "C" int fv_resample_u8_ok(int batch, int s_h, int s_w, int h_src, int w_src, int o_h, int o_w, int win_y, int win_x) {
  return launch_ok(batch, s_h, s_w) && sample_ok(s_h, s_w, h_src, w_src, o_h, o_w, win_y, win_x) ? 1 : 0;
}

extern "C" long long fv_resample_workspace_ints(int batch, int s_h, int s_w) {
  return launch_ok(batch, s_h, s_w) ? (long long)batch * sample_ws_ints(s_h, s_w) : 0;
}

extern "C" int fv_resample_coeffs(const int* plan, long long pool_bytes, int* ws, int batch, int s_h, int s_w,
                                  fv_stream_t stream) {
  FV_CHECK(plan && ws, "resample_coeffs: null pointer");
  FV_CHECK(launch_ok(batch, s_h, s_w), "resample_coeffs: batch %d, window %dx%d outside [1, 4096] x [8, 1024]^2", batch, s_h, s_w);
  FV_CHECK(pool_bytes >= 0 && (((uintptr_t)plan | (uintptr_t)ws) & 3) == 0, "resample_coeffs: negative pool size or a misaligned buffer");
  hipLaunchKernelGGL(resample_coeffs_kernel, dim3(2, batch), dim3(RS_THREADS), 0, (hipStream_t)stream, plan, pool_bytes, ws, s_h, s_w);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_resample_u8(const void* pool, long long pool_bytes, const int* plan, const int* ws, void* out, int batch,
                              int s_h, int s_w, fv_stream_t stream) {
  FV_CHECK(pool && plan && ws && out, "resample_u8: null pointer");
  FV_CHECK(launch_ok(batch, s_h, s_w), "resample_u8: batch %d, window %dx%d outside [1, 4096] x [8, 1024]^2", batch, s_h, s_w);
  FV_CHECK(pool_bytes >= 0 && (((uintptr_t)plan | (uintptr_t)ws) & 3) == 0, "resample_u8: negative pool size or a misaligned buffer");
  const int pitch = ((s_w < RS_TW ? s_w : RS_TW) + 3) & ~3;
  const int rows_cap = RS_LDS / (3 * pitch);          // >= RS_TAPS: one output row always fits
  const int out_vec = s_w % 4 == 0 && ((uintptr_t)out & 3) == 0;
  static FvOncePerDevice once;
  if (once.first())
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(resample_u8_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, RS_HDR + RS_LDS);
  const dim3 grid(fv_cdiv(s_w, RS_TW), fv_cdiv(s_h, RS_BAND), batch);
  hipLaunchKernelGGL(resample_u8_kernel, grid, dim3(RS_THREADS), (size_t)RS_HDR + (size_t)3 * rows_cap * pitch, (hipStream_t)stream,
                     (const uint8_t*)pool, plan, ws, (uint8_t*)out, pool_bytes, s_h, s_w, pitch, rows_cap, out_vec);
  FV_LAUNCH_CHECK();
  return FV_OK;
}
