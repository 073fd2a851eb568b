// hipcc-flags: -fno-fast-math -ffp-contract=off
// Device-side RandAugment of a planar uint8 batch: one layer of timm's RandAugment per pair of launches, bit for bit what
// PIL computes for the op and argument the host drew (include/fastvim_hip.h at fv_randaug_apply; restated in numpy at
// tests/randaug_ref.py).  This file is built WITHOUT fast-math and with contraction off: every operation below is the
// IEEE one, in the order written.
//
//   randaug_stats_kernel   a workgroup per (channel, sample); returns at once unless the sample's op is AUTOCONTRAST,
//                          EQUALIZE (a histogram per channel) or CONTRAST (channel 0's workgroup: the histogram of the
//                          grey value).  A histogram per wave in LDS, integer atomics; the four are added, scanned
//                          (Hillis-Steele over 256 bins) and turned into the channel's lookup table / the mean.
//   randaug_apply_kernel   a workgroup per (FV_RANDAUG_ROWS rows, sample).  The kind is read once and is uniform: no
//                          per-pixel divergence between ops.  The rows of one channel are one contiguous byte range; it
//                          is written as aligned dwords (and up to three bytes at either end), a thread per dword, the
//                          channels one after another -- the fp64 bicubic path then holds one channel's sums, not three.
//                          Loads are legal at any byte address (plane bases of odd s_h * s_w have every alignment).
//
// Nothing a plan record or the workspace holds can steer an access out of the buffers: an unknown kind copies, table
// entries are bytes, and the affine path clamps every source index into the image (a NaN coordinate takes the fill).
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int RA_THREADS = 256;
constexpr int RA_PLAN = FV_RANDAUG_PLAN_INTS;
constexpr int RA_ROWS = FV_RANDAUG_ROWS;
constexpr int RA_WS = FV_RANDAUG_WS_BYTES;

__host__ __device__ inline bool launch_ok(int batch, int s_h, int s_w, int num_layers) {
  return batch >= 1 && batch <= 4096 && s_h >= 8 && s_h <= 1024 && s_w >= 8 && s_w <= 1024 && num_layers >= 1 &&
         num_layers <= FV_RANDAUG_MAX_LAYERS;
}

// four bytes at any address: the compiler picks a load that is legal for alignment 1 (one dword load on gfx950)
__device__ __forceinline__ uint32_t ld32_unaligned(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

__device__ __forceinline__ int grey_of(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// Image.blend(degenerate, image, alpha) of one byte
__device__ __forceinline__ int blend8(int d, int i, float alpha) {
  if (alpha == 0.0f) return d;
  if (alpha == 1.0f) return i;
  const float t = (float)d + alpha * (float)(i - d);
  if (alpha >= 0.0f && alpha <= 1.0f) return (int)t & 255;
  return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

// ---------------------------------------------------------------------------------------------------------- statistics
__global__ __launch_bounds__(RA_THREADS) void randaug_stats_kernel(const uint8_t* __restrict__ in, const int* __restrict__ plan,
                                                                   uint8_t* __restrict__ ws, int s_h, int s_w, int num_layers,
                                                                   int layer) {
  __shared__ unsigned s_hist[RA_THREADS / FV_WAVE][256];
  __shared__ unsigned s_scan[256];
  __shared__ int s_lo, s_hi, s_bins;
  const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int kind = plan[((size_t)b * num_layers + layer) * RA_PLAN];
  const bool grey = kind == FV_RA_CONTRAST;
  if (grey ? c != 0 : (kind != FV_RA_AUTOCONTRAST && kind != FV_RA_EQUALIZE)) return;      // uniform in the workgroup

  for (int i = tid; i < (RA_THREADS / FV_WAVE) * 256; i += RA_THREADS) (&s_hist[0][0])[i] = 0;
  if (tid == 0) { s_lo = 256; s_hi = -1; s_bins = 0; }
  __syncthreads();

  const int n = s_h * s_w, nd = n >> 2;
  const uint8_t* p0 = in + (size_t)b * 3 * n;
  unsigned* hist = s_hist[tid / FV_WAVE];
  if (grey) {
    const uint8_t *p1 = p0 + n, *p2 = p1 + n;
    for (int i = tid; i < nd; i += RA_THREADS) {
      const uint32_t r = ld32_unaligned(p0 + 4 * i), g = ld32_unaligned(p1 + 4 * i), bl = ld32_unaligned(p2 + 4 * i);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        atomicAdd(&hist[grey_of((r >> (8 * j)) & 255, (g >> (8 * j)) & 255, (bl >> (8 * j)) & 255)], 1u);
    }
    const int i = 4 * nd + tid;
    if (i < n) atomicAdd(&hist[grey_of(p0[i], p1[i], p2[i])], 1u);
  } else {
    const uint8_t* p = p0 + (size_t)c * n;
    for (int i = tid; i < nd; i += RA_THREADS) {
      const uint32_t v = ld32_unaligned(p + 4 * i);
#pragma unroll
      for (int j = 0; j < 4; ++j) atomicAdd(&hist[(v >> (8 * j)) & 255], 1u);
    }
    const int i = 4 * nd + tid;
    if (i < n) atomicAdd(&hist[p[i]], 1u);
  }
  __syncthreads();

  // thread t owns bin t
  unsigned h = 0;
#pragma unroll
  for (int w = 0; w < RA_THREADS / FV_WAVE; ++w) h += s_hist[w][tid];
  if (h) {
    atomicMin(&s_lo, tid);
    atomicMax(&s_hi, tid);
    atomicAdd(&s_bins, 1);
  }
  // inclusive scan of h (of t * h for the grey sum: at most 255 * 2^20, no overflow)
  s_scan[tid] = grey ? h * (unsigned)tid : h;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const unsigned v = tid >= o ? s_scan[tid - o] : 0u;
    __syncthreads();
    s_scan[tid] += v;
    __syncthreads();
  }
  const int lo = s_lo, hi = s_hi;

  if (grey) {
    if (tid == 0) {
      const double mean = (double)s_scan[255] / (double)n;
      int m = (int)(mean + 0.5);
      ws[(size_t)b * RA_WS] = (uint8_t)(m < 0 ? 0 : (m > 255 ? 255 : m));
    }
    return;
  }
  int lut = tid;
  if (kind == FV_RA_AUTOCONTRAST) {
    if (hi > lo) {
      const double scale = 255.0 / (double)(hi - lo);
      const double offset = (double)(-lo) * scale;
      const double v = (double)tid * scale + offset;
      lut = (int)v;
      lut = lut < 0 ? 0 : (lut > 255 ? 255 : lut);
    }
  } else {
    // sum(histo) is the pixel count; histo[-1] the last non-empty bin
    const unsigned last = hi >= 0 ? s_scan[hi] - (hi > 0 ? s_scan[hi - 1] : 0u) : 0u;
    const unsigned step = ((unsigned)n - last) / 255u;
    if (s_bins > 1 && step != 0) {
      const unsigned q = (step / 2 + (s_scan[tid] - h)) / step;      // n before bin t: step / 2 + the bins below t
      lut = q > 255u ? 255 : (int)q;
    }
  }
  ws[(size_t)b * RA_WS + c * 256 + tid] = (uint8_t)lut;
}

// --------------------------------------------------------------------------------------------------------------- apply
// The bytes [0, n) at `o` (one channel's rows of the tile): aligned dwords from f.quad(p), the ends from f.one(p).
template <class F>
__device__ __forceinline__ void write_range(uint8_t* __restrict__ o, int n, const F& f) {
  const int tid = threadIdx.x;
  const int head = min(n, (int)((4u - (unsigned)((uintptr_t)o & 3)) & 3u));
  const int nd = (n - head) >> 2, tail = n - head - 4 * nd;
  for (int i = tid; i < nd; i += RA_THREADS) *reinterpret_cast<uint32_t*>(o + head + 4 * i) = f.quad(head + 4 * i);
  if (tid < head + tail) {
    const int p = tid < head ? tid : 4 * nd + tid;
    o[p] = (uint8_t)f.one(p);
  }
}

struct CopyOp {
  const uint8_t* in;
  __device__ __forceinline__ uint32_t quad(int p) const { return ld32_unaligned(in + p); }
  __device__ __forceinline__ int one(int p) const { return in[p]; }
};

struct LutOp {
  const uint8_t* in;
  const uint8_t* lut;      // LDS, 256 entries
  __device__ __forceinline__ uint32_t quad(int p) const {
    const uint32_t v = ld32_unaligned(in + p);
    return (uint32_t)lut[v & 255] | ((uint32_t)lut[(v >> 8) & 255] << 8) | ((uint32_t)lut[(v >> 16) & 255] << 16) |
           ((uint32_t)lut[v >> 24] << 24);
  }
  __device__ __forceinline__ int one(int p) const { return lut[in[p]]; }
};

struct ColorOp {
  const uint8_t *r, *g, *b, *self;      // the tile's rows of the three planes; self is the channel written
  float alpha;
  __device__ __forceinline__ uint32_t quad(int p) const {
    const uint32_t vr = ld32_unaligned(r + p), vg = ld32_unaligned(g + p), vb = ld32_unaligned(b + p);
    const uint32_t vs = ld32_unaligned(self + p);
    uint32_t out = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int d = grey_of((vr >> (8 * j)) & 255, (vg >> (8 * j)) & 255, (vb >> (8 * j)) & 255);
      out |= (uint32_t)blend8(d, (vs >> (8 * j)) & 255, alpha) << (8 * j);
    }
    return out;
  }
  __device__ __forceinline__ int one(int p) const { return blend8(grey_of(r[p], g[p], b[p]), self[p], alpha); }
};

// ImageFilter.SMOOTH blended with the image
struct SharpOp {
  const uint8_t* plane;      // the whole plane of the channel
  int y0, H, W;
  float alpha;
  __device__ __forceinline__ int at(int y, int x) const {
    const uint8_t* c = plane + y * W + x;
    const int i = c[0];
    if (y == 0 || y == H - 1 || x == 0 || x == W - 1) return blend8(i, i, alpha);
    const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
    float acc = 0.5f, part;
    const uint8_t* q = c + W;
    part = (float)q[-1] * k1 + (float)q[0] * k1;
    part = part + (float)q[1] * k1;
    acc = acc + part;
    part = (float)c[-1] * k1 + (float)i * k5;
    part = part + (float)c[1] * k1;
    acc = acc + part;
    q = c - W;
    part = (float)q[-1] * k1 + (float)q[0] * k1;
    part = part + (float)q[1] * k1;
    acc = acc + part;
    const int d = acc <= 0.0f ? 0 : (acc >= 255.0f ? 255 : (int)acc);
    return blend8(d, i, alpha);
  }
  __device__ __forceinline__ int one(int p) const { return at(y0 + p / W, p % W); }
  __device__ __forceinline__ uint32_t quad(int p) const {
    int y = y0 + p / W, x = p % W;
    uint32_t out = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      out |= (uint32_t)at(y, x) << (8 * j);
      if (++x == W) { x = 0; ++y; }
    }
    return out;
  }
};

__device__ __forceinline__ double cubic(double v1, double v2, double v3, double v4, double d) {
  const double p1 = v2;
  const double p2 = -v1 + v3;
  const double p3 = 2 * (v1 - v2) + v3 - v4;
  const double p4 = -v1 + v2 - v3 + v4;
  return p1 + d * (p2 + d * (p3 + d * p4));
}

// Image.transform(size, AFFINE, m, BICUBIC, fillcolor): Geometry.c's affine_transform + bicubic_filter32RGB
struct AffineOp {
  const uint8_t* plane;
  int y0, H, W, fill;
  double m0, m1, m2, m3, m4, m5;
  __device__ __forceinline__ double row(int y, int x0, double dx) const {
    const uint8_t* r = plane + min(max(y, 0), H - 1) * W;
    int a, b, c, d;
    if (x0 >= 0 && x0 + 3 < W) {
      const uint32_t v = ld32_unaligned(r + x0);
      a = v & 255; b = (v >> 8) & 255; c = (v >> 16) & 255; d = v >> 24;
    } else {
      a = r[min(max(x0, 0), W - 1)]; b = r[min(max(x0 + 1, 0), W - 1)];
      c = r[min(max(x0 + 2, 0), W - 1)]; d = r[min(max(x0 + 3, 0), W - 1)];
    }
    return cubic((double)a, (double)b, (double)c, (double)d, dx);
  }
  __device__ __forceinline__ int at(int y, int x) const {
    const double xs = (double)x + 0.5, ys = (double)y + 0.5;
    double xin = m0 * xs + m1 * ys + m2;
    double yin = m3 * xs + m4 * ys + m5;
    if (!(xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H)) return fill;
    xin -= 0.5;
    yin -= 0.5;
    const double xf = floor(xin), yf = floor(yin);
    const double dx = xin - xf, dy = yin - yf;
    const int x0 = (int)xf - 1, yy = (int)yf - 1;
    const double v1 = row(yy, x0, dx);
    const double v2 = (yy + 1 >= 0 && yy + 1 < H) ? row(yy + 1, x0, dx) : v1;
    const double v3 = (yy + 2 >= 0 && yy + 2 < H) ? row(yy + 2, x0, dx) : v2;
    const double v4 = (yy + 3 >= 0 && yy + 3 < H) ? row(yy + 3, x0, dx) : v3;
    const double v = cubic(v1, v2, v3, v4, dy);
    return v <= 0.0 ? 0 : (v >= 255.0 ? 255 : (int)v);
  }
  __device__ __forceinline__ int one(int p) const { return at(y0 + p / W, p % W); }
  __device__ __forceinline__ uint32_t quad(int p) const {
    int y = y0 + p / W, x = p % W;
    uint32_t out = 0;
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
      out |= (uint32_t)at(y, x) << (8 * j);
      if (++x == W) { x = 0; ++y; }
    }
    return out;
  }
};

__global__ __launch_bounds__(RA_THREADS) void randaug_apply_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                                   const int* __restrict__ plan, const uint8_t* __restrict__ ws,
                                                                   int s_h, int s_w, int num_layers, int layer) {
  __shared__ uint8_t s_lut[3][256];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int y0 = blockIdx.x * RA_ROWS, rows = min(RA_ROWS, s_h - y0);
  const int* rec = plan + ((size_t)b * num_layers + layer) * RA_PLAN;
  const int kind = rec[0], arg0 = rec[1], arg1 = rec[2];
  const float alpha = __int_as_float(rec[3]);
  const int n_plane = s_h * s_w, n = rows * s_w;
  const size_t base = (size_t)b * 3 * n_plane;
  const size_t tile = (size_t)y0 * s_w;

  switch (kind) {
    case FV_RA_AUTOCONTRAST:
    case FV_RA_EQUALIZE:
    case FV_RA_INVERT:
    case FV_RA_SOLARIZE:
    case FV_RA_POSTERIZE:
    case FV_RA_SOLARIZE_ADD:
    case FV_RA_BRIGHTNESS:
    case FV_RA_CONTRAST: {
      const uint8_t* w = ws + (size_t)b * RA_WS;
      int v0, v1, v2;
      if (kind == FV_RA_AUTOCONTRAST || kind == FV_RA_EQUALIZE) {
        v0 = w[tid]; v1 = w[256 + tid]; v2 = w[512 + tid];
      } else {
        int v;
        if (kind == FV_RA_INVERT) v = 255 - tid;
        else if (kind == FV_RA_SOLARIZE) v = tid < arg0 ? tid : 255 - tid;
        else if (kind == FV_RA_POSTERIZE) v = tid & ~((1 << (8 - min(max(arg0, 0), 8))) - 1);
        else if (kind == FV_RA_SOLARIZE_ADD) v = tid < arg1 ? min(max(tid + arg0, 0), 255) : tid;
        else if (kind == FV_RA_BRIGHTNESS) v = blend8(0, tid, alpha);
        else v = blend8(w[0], tid, alpha);
        v0 = v1 = v2 = v;
      }
      s_lut[0][tid] = (uint8_t)v0; s_lut[1][tid] = (uint8_t)v1; s_lut[2][tid] = (uint8_t)v2;
      __syncthreads();
#pragma unroll 1
      for (int c = 0; c < 3; ++c) {
        const size_t off = base + (size_t)c * n_plane + tile;
        write_range(out + off, n, LutOp{in + off, s_lut[c]});
      }
      break;
    }
    case FV_RA_COLOR: {
      const uint8_t* r = in + base + tile;
#pragma unroll 1
      for (int c = 0; c < 3; ++c) {
        const size_t off = base + (size_t)c * n_plane + tile;
        write_range(out + off, n, ColorOp{r, r + n_plane, r + 2 * n_plane, in + off, alpha});
      }
      break;
    }
    case FV_RA_SHARPNESS: {
#pragma unroll 1
      for (int c = 0; c < 3; ++c) {
        const size_t pl = base + (size_t)c * n_plane;
        write_range(out + pl + tile, n, SharpOp{in + pl, y0, s_h, s_w, alpha});
      }
      break;
    }
    case FV_RA_AFFINE: {
      const double* m = reinterpret_cast<const double*>(rec + 6);      // records are 72 bytes, the plan 8-byte aligned
      const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
#pragma unroll 1
      for (int c = 0; c < 3; ++c) {
        const size_t pl = base + (size_t)c * n_plane;
        write_range(out + pl + tile, n, AffineOp{in + pl, y0, s_h, s_w, (rec[4] >> (8 * c)) & 255, m0, m1, m2, m3, m4, m5});
      }
      break;
    }
    default: {
#pragma unroll 1
      for (int c = 0; c < 3; ++c) {
        const size_t off = base + (size_t)c * n_plane + tile;
        write_range(out + off, n, CopyOp{in + off});
      }
    }
  }
}

}  // namespace

extern "C" int fv_randaug_ok(int batch, int s_h, int s_w, int num_layers) { return launch_ok(batch, s_h, s_w, num_layers) ? 1 : 0; }

extern "C" long long fv_randaug_workspace_bytes(int batch) { return batch >= 1 && batch <= 4096 ? (long long)batch * RA_WS : 0; }

extern "C" int fv_randaug_stats(const void* in, const int* plan, void* ws, int batch, int s_h, int s_w, int num_layers,
                                int layer, fv_stream_t stream) {
  FV_CHECK(in && plan && ws, "randaug_stats: null pointer");
  FV_CHECK(launch_ok(batch, s_h, s_w, num_layers), "randaug_stats: batch %d, %dx%d images, %d layers outside [1, 4096] x [8, 1024]^2 x [1, %d]",
           batch, s_h, s_w, num_layers, FV_RANDAUG_MAX_LAYERS);
  FV_CHECK(layer >= 0 && layer < num_layers, "randaug_stats: layer %d of %d", layer, num_layers);
  FV_CHECK(((uintptr_t)plan & 7) == 0, "randaug_stats: the plan must be 8-byte aligned");
  hipLaunchKernelGGL(randaug_stats_kernel, dim3(3, batch), dim3(RA_THREADS), 0, (hipStream_t)stream, (const uint8_t*)in, plan,
                     (uint8_t*)ws, s_h, s_w, num_layers, layer);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_randaug_apply(const void* in, void* out, const int* plan, const void* ws, int batch, int s_h, int s_w,
                                int num_layers, int layer, fv_stream_t stream) {
  FV_CHECK(in && out && plan && ws, "randaug_apply: null pointer");
  FV_CHECK(launch_ok(batch, s_h, s_w, num_layers), "randaug_apply: batch %d, %dx%d images, %d layers outside [1, 4096] x [8, 1024]^2 x [1, %d]",
           batch, s_h, s_w, num_layers, FV_RANDAUG_MAX_LAYERS);
  FV_CHECK(layer >= 0 && layer < num_layers, "randaug_apply: layer %d of %d", layer, num_layers);
  FV_CHECK(((uintptr_t)plan & 7) == 0, "randaug_apply: the plan must be 8-byte aligned");
  const uintptr_t a = (uintptr_t)in, o = (uintptr_t)out, bytes = (uintptr_t)batch * 3 * s_h * s_w;
  FV_CHECK(a + bytes <= o || o + bytes <= a, "randaug_apply: in and out overlap");
  hipLaunchKernelGGL(randaug_apply_kernel, dim3(fv_cdiv(s_h, RA_ROWS), batch), dim3(RA_THREADS), 0, (hipStream_t)stream,
                     (const uint8_t*)in, (uint8_t*)out, plan, (const uint8_t*)ws, s_h, s_w, num_layers, layer);
  FV_LAUNCH_CHECK();
  return FV_OK;
}
