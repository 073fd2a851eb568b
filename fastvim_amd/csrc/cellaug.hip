// hipcc-flags: -fno-fast-math -ffp-contract=off
// Device-side cell-image augmentation of the channel models' loader: the pixel work of the reference's
// CellAugmentation(is_train=True) (cell_imaging/transformations/cell.py:104-149) in front of A.Normalize, on planar uint8
// planes (include/fastvim_hip.h at fv_cellaug_geom; restated in numpy at tests/cellaug_ref.py).
//
//   cellaug_geom_kernel     a thread owns four neighbouring pixels of one row of the S x S crop and walks the channels: the
//                           geometry (pad + crop offset, index mirror, or the four reflected taps and 5-bit fractions of a
//                           rotation) is worked out once and reused for every plane.  A rotation is the fixed-point scheme
//                           of an 8-bit bilinear warpAffine: fp64 products, rint, then integers only.  One gather per tap
//                           from the staged source; there is no intermediate crop in memory.
//   cellaug_filter_kernel   a workgroup of 128 threads owns a 32 x 32 tile of one plane (224 = 7 x 32: no idle lanes at the
//                           recipe's size).  With defocus it keeps the tile and a halo of 4 (reflect-101 at the plane's
//                           borders) in LDS as bytes, 40 rows of 40 B: a thread owns four neighbouring pixels of rows r and
//                           r + 16 and reads, per tap row, the twelve bytes the four share as three dwords (rows 10 dwords
//                           apart: the 32 lanes of a half-wave touch 32 different banks).  A row of nine weights comes out
//                           of LDS in one go (three 16-byte broadcasts) and serves all eight pixels; each is made
//                           wave-uniform, and an exact zero is skipped by a scalar branch.  Taps in row-major order, fp32,
//                           product and add rounded separately -- this file is built WITHOUT fast-math and with contraction
//                           off.  1,600 + 432 + 256 B of LDS: occupancy is not LDS-bound.  Without defocus the tile is a
//                           straight copy (the branch is the same for the whole workgroup).  The sample's holes are zeroed
//                           on the way out.
//
// Every output byte has exactly one owner lane in either launch: no atomics, nothing to clear before a replay.  A record
// that is out of range (source outside the pool, sides outside [1, 4096]) reads nothing and gives zeros.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int CA_PLAN = FV_CELLAUG_PLAN_INTS;
constexpr int CA_TAPS = FV_CELLAUG_TAPS;               // 9: the defocus support served
constexpr int CA_HALO = CA_TAPS / 2;
constexpr int CA_MAX_HOLES = FV_CELLAUG_MAX_HOLES;
constexpr int CA_THREADS = 256;                        // geometry launch
constexpr int CA_TW = 32, CA_TH = 32;                  // filter tile
constexpr int CA_FTHREADS = CA_TW / 4 * CA_TH / 2;     // 128: four pixels of two rows per thread
constexpr int CA_PITCH = CA_TW + 2 * CA_HALO;          // 40 B = 10 dwords
constexpr int CA_ROWS = CA_TH + 2 * CA_HALO;           // 40
constexpr int CA_WROW = 12;                            // floats per weight row in LDS (9 used)
// words of a record
constexpr int CA_OFF = 0, CA_H = 2, CA_W = 3, CA_OY = 4, CA_OX = 5, CA_OP = 6, CA_DEFOCUS = 7, CA_NHOLES = 8;
constexpr int CA_MATRIX = 12, CA_KERNEL = 24, CA_HOLES = 108;
static_assert(CA_HOLES + 4 * CA_MAX_HOLES <= CA_PLAN && CA_KERNEL + CA_TAPS * CA_TAPS <= CA_HOLES, "record layout");

__host__ __device__ inline bool launch_ok(int batch, int channels, int size) {
  return batch >= 1 && batch <= 4096 && channels >= 1 && channels <= 16 && size >= 8 && size <= 512;
}

// BORDER_REFLECT_101 for any index (n >= 2): ... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ...
__device__ __forceinline__ int reflect101(int i, int n) {
  if ((unsigned)i < (unsigned)n) return i;
  const int p = 2 * (n - 1);
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - i;
}

// rint to int32 of a value that is far inside the int range for every record the host writes; the clamp only keeps a
// corrupt record's arithmetic defined (taps are reflected into the crop whatever comes out)
__device__ __forceinline__ int rint_i32(double v) {
  v = fmin(fmax(v, -536870912.0), 536870912.0);
  return (int)rint(v);
}

__device__ __forceinline__ void store4(uint8_t* dst, uint32_t v, int n, int vec) {
  if (vec) {
    *reinterpret_cast<uint32_t*>(dst) = v;
  } else {
    for (int j = 0; j < n; ++j) dst[j] = (uint8_t)(v >> (8 * j));
  }
}

__global__ __launch_bounds__(CA_THREADS) void cellaug_geom_kernel(const uint8_t* __restrict__ pool, long long pool_bytes,
                                                                  const int* __restrict__ plan, uint8_t* __restrict__ out,
                                                                  int C, int S, int G, int vec) {
  const int b = blockIdx.y;
  const int idx = blockIdx.x * CA_THREADS + threadIdx.x;
  if (idx >= S * G) return;
  const int y = idx / G, x = (idx - y * G) * 4;
  const int nx = min(4, S - x);
  const int* rec = plan + (size_t)b * CA_PLAN;
  const long long off = (long long)(((unsigned long long)(unsigned)rec[CA_OFF + 1] << 32) | (unsigned long long)(unsigned)rec[CA_OFF]);
  const int H = rec[CA_H], W = rec[CA_W], oy = rec[CA_OY], ox = rec[CA_OX], op = rec[CA_OP];
  bool valid = H >= 1 && H <= 4096 && W >= 1 && W <= 4096 && oy >= -8192 && oy <= 8192 && ox >= -8192 && ox <= 8192;
  valid = valid && op >= 0 && op <= 3 && off >= 0 && off <= pool_bytes && (long long)C * H * W <= pool_bytes - off;
  const size_t plane_src = (size_t)H * W, plane_dst = (size_t)S * S;
  const uint8_t* src = pool + (valid ? off : 0);
  uint8_t* dst = out + ((size_t)b * C * S + y) * S + x;

  if (!valid || op != FV_CELLAUG_ROTATE) {
    int o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int xx = x + j;
      const int cy = op == FV_CELLAUG_VFLIP ? S - 1 - y : y, cx = op == FV_CELLAUG_HFLIP ? S - 1 - xx : xx;
      const int sy = cy - oy, sx = cx - ox;
      o[j] = valid && xx < S && sy >= 0 && sy < H && sx >= 0 && sx < W ? sy * W + sx : -1;
    }
    // four source pixels in a row (mirrored or not) are one load, legal at any byte address
    const bool run = o[0] >= 0 && o[3] >= 0;
    const int first = min(o[0], o[3]);
    for (int c = 0; c < C; ++c) {
      const uint8_t* s = src + c * plane_src;
      uint32_t v = 0;
      if (run) {
        __builtin_memcpy(&v, s + first, 4);
        if (o[3] < o[0]) v = __builtin_bswap32(v);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (o[j] >= 0) v |= (uint32_t)s[o[j]] << (8 * j);
      }
      store4(dst + c * plane_dst, v, nx, vec);
    }
    return;
  }

  const double* m = reinterpret_cast<const double*>(rec + CA_MATRIX);
  const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
  const int X0 = rint_i32((m1 * (double)y + m2) * 1024.0) + 16;
  const int Y0 = rint_i32((m4 * (double)y + m5) * 1024.0) + 16;
  int o[4][4], fx[4], fy[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int xx = x + j;
    const int X = (X0 + rint_i32(m0 * (double)xx * 1024.0)) >> 5;
    const int Y = (Y0 + rint_i32(m3 * (double)xx * 1024.0)) >> 5;
    const int sx = X >> 5, sy = Y >> 5;
    fx[j] = X & 31;
    fy[j] = Y & 31;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int ry = reflect101(sy + (t >> 1), S) - oy, rx = reflect101(sx + (t & 1), S) - ox;
      o[j][t] = xx < S && ry >= 0 && ry < H && rx >= 0 && rx < W ? ry * W + rx : -1;
    }
  }
  for (int c = 0; c < C; ++c) {
    const uint8_t* s = src + c * plane_src;
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int p[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) p[t] = o[j][t] >= 0 ? (int)s[o[j][t]] : 0;
      const int ax = fx[j], ay = fy[j];
      const int acc = p[0] * ((32 - ay) * (32 - ax) * 32) + p[1] * ((32 - ay) * ax * 32) + p[2] * (ay * (32 - ax) * 32) +
                      p[3] * (ay * ax * 32);
      v |= (uint32_t)((acc + 16384) >> 15) << (8 * j);
    }
    store4(dst + c * plane_dst, v, nx, vec);
  }
}

__device__ __forceinline__ float uniform_f32(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// the twelve bytes that four neighbouring pixels' nine taps of one row share, as floats
__device__ __forceinline__ void row12(const uint8_t* tile_row, int tx, float* p) {
  const uint32_t* row = reinterpret_cast<const uint32_t*>(tile_row) + tx;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const uint32_t d = row[q];
#pragma unroll
    for (int i = 0; i < 4; ++i) p[4 * q + i] = (float)((d >> (8 * i)) & 0xffu);
  }
}

__global__ __launch_bounds__(CA_FTHREADS) void cellaug_filter_kernel(const uint8_t* __restrict__ in, const int* __restrict__ plan,
                                                                    uint8_t* __restrict__ out, int C, int S, int tiles_x,
                                                                    int vec) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[CA_ROWS * CA_PITCH];
  __shared__ __attribute__((aligned(16))) float s_w[CA_TAPS * CA_WROW];
  __shared__ int s_holes[4 * CA_MAX_HOLES];
  const int tid = threadIdx.x, b = blockIdx.y, c = blockIdx.z;
  const int ty0 = blockIdx.x / tiles_x;
  const int y0 = ty0 * CA_TH, x0 = (blockIdx.x - ty0 * tiles_x) * CA_TW;
  const int* rec = plan + (size_t)b * CA_PLAN;
  const bool defocus = rec[CA_DEFOCUS] != 0;
  const int nh = min(max(rec[CA_NHOLES], 0), CA_MAX_HOLES);
  const size_t base = ((size_t)b * C + c) * S * S;
  const uint8_t* src = in + base;
  uint8_t* dst = out + base;

  if (tid < 4 * nh) s_holes[tid] = rec[CA_HOLES + tid];
  if (defocus) {
    // a row of weights is padded to twelve floats: read back as three 16-byte broadcasts
    if (tid < CA_TAPS * CA_TAPS) s_w[tid / CA_TAPS * CA_WROW + tid % CA_TAPS] = __int_as_float(rec[CA_KERNEL + tid]);
    // the tile with its halo, a dword at a time: one load where the four bytes lie inside a row of an aligned plane
    for (int i = tid; i < CA_ROWS * (CA_PITCH / 4); i += CA_FTHREADS) {
      const int r = i / (CA_PITCH / 4), q = i - r * (CA_PITCH / 4);
      const int gy = reflect101(y0 - CA_HALO + r, S), gx = x0 - CA_HALO + 4 * q;
      const uint8_t* row = src + (size_t)gy * S;
      uint32_t v;
      if (vec && gx >= 0 && gx + 3 < S) {
        v = *reinterpret_cast<const uint32_t*>(row + gx);
      } else {
        v = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) v |= (uint32_t)row[reflect101(gx + j, S)] << (8 * j);
      }
      reinterpret_cast<uint32_t*>(tile)[i] = v;
    }
  }
  __syncthreads();

  // a thread owns four neighbouring pixels of rows ty and ty + CA_TH / 2: a weight is fetched once for all eight
  const int tx = tid % (CA_TW / 4), ty = tid / (CA_TW / 4);
  const int x = x0 + 4 * tx;
  if (x >= S || y0 + ty >= S) return;
  const int nx = min(4, S - x);
  uint32_t v[2] = {0, 0};
  if (defocus) {
    float acc[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll 1
    for (int ky = 0; ky < CA_TAPS; ++ky) {
      float w[CA_WROW], p[2][12];
      const float4* wr = reinterpret_cast<const float4*>(s_w + ky * CA_WROW);
#pragma unroll
      for (int q = 0; q < CA_WROW / 4; ++q) {
        const float4 t = wr[q];
        w[4 * q] = t.x; w[4 * q + 1] = t.y; w[4 * q + 2] = t.z; w[4 * q + 3] = t.w;
      }
      row12(tile + (ty + ky) * CA_PITCH, tx, p[0]);
      row12(tile + (ty + CA_TH / 2 + ky) * CA_PITCH, tx, p[1]);
#pragma unroll
      for (int kx = 0; kx < CA_TAPS; ++kx) {
        const float wk = uniform_f32(w[kx]);
        if (wk != 0.f) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float t = p[h][j + kx] * wk;
              acc[h][j] = acc[h][j] + t;
            }
          }
        }
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float r = fminf(fmaxf(rintf(acc[h][j]), 0.f), 255.f);
        v[h] |= (uint32_t)(int)r << (8 * j);
      }
    }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int y = y0 + ty + h * (CA_TH / 2);
    if (y >= S) break;
    if (!defocus) {
      if (vec) {
        v[h] = *reinterpret_cast<const uint32_t*>(src + (size_t)y * S + x);
      } else {
        for (int j = 0; j < nx; ++j) v[h] |= (uint32_t)src[(size_t)y * S + x + j] << (8 * j);
      }
    }
    for (int k = 0; k < nh; ++k) {
      const int hy1 = s_holes[4 * k], hx1 = s_holes[4 * k + 1], hy2 = s_holes[4 * k + 2], hx2 = s_holes[4 * k + 3];
      if (y >= hy1 && y < hy2) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x + j >= hx1 && x + j < hx2) v[h] &= ~(0xffu << (8 * j));
      }
    }
    store4(dst + (size_t)y * S + x, v[h], nx, vec);
  }
}

}  // namespace

extern "C" int fv_cellaug_geom(const void* pool, long long pool_bytes, const int* plan, void* out, int batch, int channels,
                               int size, fv_stream_t stream) {
  FV_CHECK(pool && plan && out, "cellaug_geom: null pointer");
  FV_CHECK(launch_ok(batch, channels, size), "cellaug_geom: batch %d, channels %d, size %d outside [1, 4096] x [1, 16] x [8, 512]",
           batch, channels, size);
  FV_CHECK(pool_bytes >= 0 && ((uintptr_t)plan & 7) == 0, "cellaug_geom: negative pool size or a plan table that is not 8-byte aligned");
  const int G = fv_cdiv(size, 4);
  const int vec = size % 4 == 0 && ((uintptr_t)out & 3) == 0;
  hipLaunchKernelGGL(cellaug_geom_kernel, dim3(fv_cdiv((long)size * G, CA_THREADS), batch), dim3(CA_THREADS), 0, (hipStream_t)stream,
                     (const uint8_t*)pool, pool_bytes, plan, (uint8_t*)out, channels, size, G, vec);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_cellaug_filter(const void* in, const int* plan, void* out, int batch, int channels, int size, fv_stream_t stream) {
  FV_CHECK(in && plan && out, "cellaug_filter: null pointer");
  FV_CHECK(launch_ok(batch, channels, size), "cellaug_filter: batch %d, channels %d, size %d outside [1, 4096] x [1, 16] x [8, 512]",
           batch, channels, size);
  FV_CHECK(((uintptr_t)plan & 7) == 0, "cellaug_filter: the plan table is not 8-byte aligned");
  const size_t n = (size_t)batch * channels * size * size;
  const uintptr_t a = (uintptr_t)in, o = (uintptr_t)out;
  FV_CHECK(a + n <= o || o + n <= a, "cellaug_filter: in and out overlap (a tile reads its neighbours' halo)");
  const int vec = size % 4 == 0 && ((a | o) & 3) == 0;
  const int tiles_x = fv_cdiv(size, CA_TW), tiles_y = fv_cdiv(size, CA_TH);
  hipLaunchKernelGGL(cellaug_filter_kernel, dim3(tiles_x * tiles_y, batch, channels), dim3(CA_FTHREADS), 0, (hipStream_t)stream,
                     (const uint8_t*)in, plan, (uint8_t*)out, channels, size, tiles_x, vec);
  FV_LAUNCH_CHECK();
  return FV_OK;
}
