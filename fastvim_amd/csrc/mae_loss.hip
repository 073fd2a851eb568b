// The MAE reconstruction loss (models/mae/models_mamba_faster_mae_vimdecoder.py:864-880, restated at oracle/model.py:429-437)
// as two launches forward and one backward, for fp32 images and for uint8 images with the (3, 256) fp32 normalisation table:
//   mae_loss_rows_kernel    one WAVE per patch (n, l), four patches per workgroup.  A patch with mask == 0 writes
//                           loss_rows = 0, row_stats = (0, 0) and reads neither the image nor pred.  Otherwise the wave loads
//                           its patch in IMAGE order (lanes walk px fastest: the (c, py) segments of p pixels are contiguous),
//                           stores every value into its LDS slab at j = (py p + px) 3 + c -- the "nhwpqc" order of pred --,
//                           takes the mean (a sum, then the sum of the residuals added to it) and then the centred second
//                           moment from the slab (exact fp32 passes, never E[t^2] - mean^2; wave reductions only), and
//                           streams pred against 16-byte reads of the slab.
//   mae_loss_final_kernel   ONE workgroup of 1024: sum(loss_rows mask) and sum(mask) in fp64 in a fixed order (eval.hip's scheme), no
//                           atomics: the same inputs give the same bits.
//   mae_loss_bwd_kernel     the same mapping; target is RECOMPUTED from the image and the saved (mean, rstd);
//                           dpred = g mask 2 (pred - target) / (D sum(mask)) in pred's type, zeros (nothing read) where mask == 0.
//
// The two image sources are one template in which only the pixel fetch differs: the uint8 form looks table[c][v] up in an
// LDS copy of the table (no arithmetic on the byte: fastvim_amd/pixels.py) and from the slab on runs the code of the float
// form, so it equals the float form on lookup(table, img) bit for bit.  Floating-point reassociation and contraction are
// switched off for the whole file: every sum below has ONE order, the one written.
//
// Alignment: img and pred need only the alignment of their element type.  The image is loaded 4, 2 or 1 pixels at a time
// (16 / 8 / 4 B of fp32, 4 / 2 / 1 B of uint8) and pred / dpred 4, 2 or 1 elements at a time, each chosen on the host from the
// patch width and the actual base address (patch 14: 56-byte fp32 and 14-byte uint8 segments, bf16 rows of 1176 B).
// LDS: the table (3 KB) + 4 slabs of D floats; slab stores have a lane stride of 3 IV dwords, and a 32-lane group holds all
// three channels (rows are walked channel-fastest), which keeps them at most 2-way conflicting.
#include "common.h"

#pragma clang fp reassociate(off) contract(off)

namespace {

constexpr int ML_WAVES = 4;               // patches per workgroup
constexpr int ML_TABLE_FLOATS = 3 * 256;
constexpr int ML_MAX_PATCH = 28;          // D = 2352: 4 slabs + the table = 40 KB
constexpr long ML_MAX_PATCHES = 128L * 1024;

typedef uint32_t ml_u32x2 __attribute__((ext_vector_type(2)));

// ---- the patch of image n at grid cell (gy, gx) -> slab[(py p + px) 3 + c].  `org`: element offset of pixel (c = 0, py = 0,
// px = 0).  IV pixels per load; the host guarantees p % IV == 0 and IV-element alignment of every segment start.
template <bool U8, int IV>
__device__ __forceinline__ void load_patch(const void* __restrict__ img, const float* tab, float* slab, size_t org, int H, int W,
                                           int p, int lane) {
  const int upr = p / IV;                 // loads per (c, py) row segment
  const int units = 3 * p * upr;
  for (int u = lane; u < units; u += FV_WAVE) {
    const int row = u / upr, x = (u - row * upr) * IV;
    const int py = row / 3, c = row - py * 3;
    const size_t off = org + ((size_t)c * H + py) * W + x;
    float v[IV];
    if constexpr (U8) {
      const uint8_t* s = reinterpret_cast<const uint8_t*>(img) + off;
      const float* trow = tab + c * 256;
      uint32_t w;                         // bytes are UNSIGNED: shifts and masks of an unsigned word
      if constexpr (IV == 4) w = *reinterpret_cast<const uint32_t*>(s);
      else if constexpr (IV == 2) w = *reinterpret_cast<const uint16_t*>(s);
      else w = *s;
#pragma unroll
      for (int k = 0; k < IV; ++k) v[k] = trow[(w >> (8 * k)) & 0xffu];
    } else {
      const float* s = reinterpret_cast<const float*>(img) + off;
      if constexpr (IV == 4) {
        const float4 t = *reinterpret_cast<const float4*>(s);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
      } else if constexpr (IV == 2) {
        const float2 t = *reinterpret_cast<const float2*>(s);
        v[0] = t.x; v[1] = t.y;
      } else {
        v[0] = *s;
      }
    }
    float* d = slab + (py * p + x) * 3 + c;
#pragma unroll
    for (int k = 0; k < IV; ++k) d[3 * k] = v[k];
  }
}

template <bool U8>
__device__ __forceinline__ void load_patch_iv(const void* __restrict__ img, const float* tab, float* slab, size_t org, int H, int W,
                                              int p, int lane, int iv) {
  if (iv == 4) load_patch<U8, 4>(img, tab, slab, org, H, W, p, lane);
  else if (iv == 2) load_patch<U8, 2>(img, tab, slab, org, H, W, p, lane);
  else load_patch<U8, 1>(img, tab, slab, org, H, W, p, lane);
  // the slab is written and read by this wave only
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- four consecutive elements of a pred / dpred row, pv (4, 2 or 1) elements per access
__device__ __forceinline__ void ld4(const float* p, int pv, float (&v)[4]) {
  if (pv == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else if (pv == 2) {
    const float2 a = *reinterpret_cast<const float2*>(p), b = *reinterpret_cast<const float2*>(p + 2);
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
  } else {
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
  }
}
__device__ __forceinline__ void ld4(const bf16_t* p, int pv, float (&v)[4]) {
  uint32_t lo, hi;
  if (pv == 4) {
    const ml_u32x2 t = *reinterpret_cast<const ml_u32x2*>(p);
    lo = t.x; hi = t.y;
  } else if (pv == 2) {
    lo = *reinterpret_cast<const uint32_t*>(p);
    hi = *reinterpret_cast<const uint32_t*>(p + 2);
  } else {
    const uint16_t* q = reinterpret_cast<const uint16_t*>(p);
    lo = (uint32_t)q[0] | ((uint32_t)q[1] << 16);
    hi = (uint32_t)q[2] | ((uint32_t)q[3] << 16);
  }
  v[0] = __uint_as_float(lo << 16); v[1] = __uint_as_float(lo & 0xffff0000u);
  v[2] = __uint_as_float(hi << 16); v[3] = __uint_as_float(hi & 0xffff0000u);
}
__device__ __forceinline__ void st4(float* p, int pv, const float (&v)[4]) {
  if (pv == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else if (pv == 2) {
    *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
    *reinterpret_cast<float2*>(p + 2) = make_float2(v[2], v[3]);
  } else {
    p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3];
  }
}
__device__ __forceinline__ void st4(bf16_t* p, int pv, const float (&v)[4]) {
  const uint32_t lo = pack_bf16x2(v[0], v[1]), hi = pack_bf16x2(v[2], v[3]);      // round to nearest even
  if (pv == 4) {
    ml_u32x2 t;
    t.x = lo; t.y = hi;
    *reinterpret_cast<ml_u32x2*>(p) = t;
  } else if (pv == 2) {
    *reinterpret_cast<uint32_t*>(p) = lo;
    *reinterpret_cast<uint32_t*>(p + 2) = hi;
  } else {
    uint16_t* q = reinterpret_cast<uint16_t*>(p);
    q[0] = (uint16_t)lo; q[1] = (uint16_t)(lo >> 16); q[2] = (uint16_t)hi; q[3] = (uint16_t)(hi >> 16);
  }
}

struct Geom {
  int H, W, p, gw, L, D;      // image, patch, grid width, patches per image, elements per patch
  int iv, pv;                 // pixels per image load, elements per pred access
  long rows;                  // batch * L
};

// the table -> LDS (uint8 form), then this wave's patch index and slab; false: no patch for this wave
template <bool U8>
__device__ __forceinline__ void stage_table(float* tab, const float* __restrict__ table) {
  if constexpr (U8) {
    for (int e = threadIdx.x; e < ML_TABLE_FLOATS / 4; e += blockDim.x)
      reinterpret_cast<float4*>(tab)[e] = reinterpret_cast<const float4*>(table)[e];
    __syncthreads();
  }
}

__device__ __forceinline__ size_t patch_origin(const Geom& G, long row) {
  const long n = row / G.L;
  const int l = (int)(row - n * G.L);
  const int gy = l / G.gw, gx = l - gy * G.gw;
  return ((size_t)n * 3 * G.H + (size_t)gy * G.p) * G.W + (size_t)gx * G.p;
}

// ---- forward rows
template <typename TP, bool U8>
__global__ __launch_bounds__(256) void mae_loss_rows_kernel(const void* __restrict__ img, const float* __restrict__ table,
                                                            const TP* __restrict__ pred, const float* __restrict__ mask,
                                                            float* __restrict__ loss_rows, float* __restrict__ row_stats, Geom G,
                                                            int norm_pix, float inv_d, float inv_dm1) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* tab = reinterpret_cast<float*>(smem);
  stage_table<U8>(tab, table);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * ML_WAVES + wave;
  if (row >= G.rows) return;
  if (mask[row] == 0.f) {                 // wave-uniform: nothing of this patch is read
    if (lane == 0) {
      loss_rows[row] = 0.f;
      row_stats[2 * row] = 0.f;
      row_stats[2 * row + 1] = 0.f;
    }
    return;
  }
  float* slab = tab + ML_TABLE_FLOATS + wave * G.D;
  load_patch_iv<U8>(img, tab, slab, patch_origin(G, row), G.H, G.W, G.p, lane, G.iv);
  const int D = G.D;
  float mean = 0.f, rstd = 1.f;           // target = t exactly without norm_pix: (t - 0) * 1
  if (norm_pix) {
    float s = 0.f;
    for (int j = lane * 4; j < D; j += 4 * FV_WAVE) {
      const float4 t = *reinterpret_cast<const float4*>(slab + j);
      s += (t.x + t.y) + (t.z + t.w);
    }
    mean = wave_sum(s) * inv_d;
    // The mean once more, from the residuals: rstd is up to 1000 (eps 1e-6), so one rounding of the mean of a flat patch
    // would show as a target of 1e-4 where the exact one is 0.  On a constant patch t - mean is exact and the sum restores t.
    float r = 0.f;
    for (int j = lane * 4; j < D; j += 4 * FV_WAVE) {
      const float4 t = *reinterpret_cast<const float4*>(slab + j);
      r += ((t.x - mean) + (t.y - mean)) + ((t.z - mean) + (t.w - mean));
    }
    mean = mean + wave_sum(r) * inv_d;
    float q = 0.f;
    for (int j = lane * 4; j < D; j += 4 * FV_WAVE) {
      const float4 t = *reinterpret_cast<const float4*>(slab + j);
      const float a = t.x - mean, b = t.y - mean, c = t.z - mean, d = t.w - mean;
      q += (a * a + b * b) + (c * c + d * d);
    }
    rstd = rsqrtf(wave_sum(q) * inv_dm1 + 1.0e-6f);
  }
  const TP* prow = pred + (size_t)row * D;
  float acc = 0.f;
  for (int j = lane * 4; j < D; j += 4 * FV_WAVE) {
    const float4 t = *reinterpret_cast<const float4*>(slab + j);
    float pr[4];
    ld4(prow + j, G.pv, pr);
    const float a = pr[0] - (t.x - mean) * rstd, b = pr[1] - (t.y - mean) * rstd;
    const float c = pr[2] - (t.z - mean) * rstd, d = pr[3] - (t.w - mean) * rstd;
    acc += (a * a + b * b) + (c * c + d * d);
  }
  acc = wave_sum(acc) * inv_d;
  if (lane == 0) {
    loss_rows[row] = acc;
    row_stats[2 * row] = mean;
    row_stats[2 * row + 1] = rstd;
  }
}

// ---- forward final: one workgroup of 1024.  Thread t sums rows 4 (t + 1024 k) .. + 3, k = 0, 1, ..., in that order in fp64
// (16-byte loads where both arrays are 16-byte aligned, single ones else: the order is the same), then the butterfly over
// the wave, then the sixteen waves as a fixed tree.
constexpr int ML_FINAL_THREADS = 1024;

__device__ __forceinline__ void ld_rows4(const float* p, long r, long rows, bool vec, float (&v)[4]) {
  if (vec && r + 4 <= rows) {
    const float4 t = *reinterpret_cast<const float4*>(p + r);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = r + k < rows ? p[r + k] : 0.f;
  }
}

__global__ __launch_bounds__(ML_FINAL_THREADS) void mae_loss_final_kernel(const float* __restrict__ loss_rows,
                                                                          const float* __restrict__ mask, float* __restrict__ out,
                                                                          long rows, int vec) {
  __shared__ double s_l[ML_FINAL_THREADS / FV_WAVE], s_m[ML_FINAL_THREADS / FV_WAVE];
  const int tid = threadIdx.x;
  double sl = 0.0, sm = 0.0;
#pragma unroll 2
  for (long r = 4L * tid; r < rows; r += 4L * ML_FINAL_THREADS) {
    float l[4], m[4];
    ld_rows4(loss_rows, r, rows, vec != 0, l);
    ld_rows4(mask, r, rows, vec != 0, m);
#pragma unroll
    for (int k = 0; k < 4; ++k) {         // (a row past the end adds 0 * 0 and 0)
      sl += (double)(l[k] * m[k]);
      sm += (double)m[k];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sl += __shfl_xor(sl, o);
    sm += __shfl_xor(sm, o);
  }
  if ((tid & 63) == 0) {
    s_l[tid >> 6] = sl;
    s_m[tid >> 6] = sm;
  }
  __syncthreads();
  if (tid == 0) {
    double tl[16], tm[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) { tl[k] = s_l[k]; tm[k] = s_m[k]; }
#pragma unroll
    for (int w = 8; w > 0; w >>= 1) {
#pragma unroll
      for (int k = 0; k < w; ++k) { tl[k] = tl[2 * k] + tl[2 * k + 1]; tm[k] = tm[2 * k] + tm[2 * k + 1]; }
    }
    out[0] = (float)(tl[0] / tm[0]);
    out[1] = (float)tm[0];
  }
}

// ---- backward
template <typename TP, bool U8>
__global__ __launch_bounds__(256) void mae_loss_bwd_kernel(const void* __restrict__ img, const float* __restrict__ table,
                                                           const TP* __restrict__ pred, const float* __restrict__ mask,
                                                           const float* __restrict__ row_stats, const float* __restrict__ sum_mask,
                                                           const float* __restrict__ g, TP* __restrict__ dpred, Geom G,
                                                           float two_inv_d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* tab = reinterpret_cast<float*>(smem);
  stage_table<U8>(tab, table);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * ML_WAVES + wave;
  if (row >= G.rows) return;
  const int D = G.D;
  TP* drow = dpred + (size_t)row * D;
  const float m = mask[row];
  if (m == 0.f) {                         // wave-uniform: zeros, nothing read
    const float z[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = lane * 4; j < D; j += 4 * FV_WAVE) st4(drow + j, G.pv, z);
    return;
  }
  float* slab = tab + ML_TABLE_FLOATS + wave * D;
  load_patch_iv<U8>(img, tab, slab, patch_origin(G, row), G.H, G.W, G.p, lane, G.iv);
  const float mean = row_stats[2 * row], rstd = row_stats[2 * row + 1];
  const float scale = ((g[0] * m) * two_inv_d) / sum_mask[0];
  const TP* prow = pred + (size_t)row * D;
  for (int j = lane * 4; j < D; j += 4 * FV_WAVE) {
    const float4 t = *reinterpret_cast<const float4*>(slab + j);
    float pr[4];
    ld4(prow + j, G.pv, pr);
    const float o[4] = {scale * (pr[0] - (t.x - mean) * rstd), scale * (pr[1] - (t.y - mean) * rstd),
                        scale * (pr[2] - (t.z - mean) * rstd), scale * (pr[3] - (t.w - mean) * rstd)};
    st4(drow + j, G.pv, o);
  }
}

// ---- host side
bool shape_ok(int batch, int chans, int height, int width, int patch, int pred_dtype) {
  if (batch <= 0 || chans != 3 || height <= 0 || height != width) return false;
  if (patch < 8 || patch > ML_MAX_PATCH || patch % 2 != 0 || height % patch != 0) return false;
  if (pred_dtype != FV_F32 && pred_dtype != FV_BF16) return false;
  const long L = (long)(height / patch) * (width / patch);
  return (long)batch * L <= ML_MAX_PATCHES;
}

// pixels per image load: every (c, py) segment starts at base + (a multiple of W) + (a multiple of patch) elements
int image_vec(const void* img, bool u8, int width, int patch) {
  const size_t esz = u8 ? 1 : 4;
  for (int iv = 4; iv > 1; iv >>= 1)
    if (patch % iv == 0 && width % iv == 0 && ((uintptr_t)img % (iv * esz)) == 0) return iv;
  return 1;
}

// elements per pred access: a row is D elements, D % 4 == 0, so only the base address decides
int pred_vec(const void* a, const void* b, int dtype) {
  const size_t esz = dtype == FV_F32 ? 4 : 2;
  const uintptr_t bits = (uintptr_t)a | (uintptr_t)b;
  return bits % (4 * esz) == 0 ? 4 : bits % (2 * esz) == 0 ? 2 : 1;
}

int check_common(const char* what, const void* img, const float* table, const void* pred, int pred_dtype, const float* mask,
                 int batch, int height, int width, int patch) {
  FV_CHECK(img && pred && mask, "%s: null pointer", what);
  FV_CHECK(shape_ok(batch, 3, height, width, patch, pred_dtype),
           "%s: unsupported shape (batch %d, %dx%d, patch %d, pred dtype code %d): square 3-channel images of whole patches, patch "
           "even in [8, %d], pred fp32 or bf16, at most %ld patches", what, batch, height, width, patch, pred_dtype, ML_MAX_PATCH,
           ML_MAX_PATCHES);
  FV_CHECK(((uintptr_t)mask & 3) == 0 && ((uintptr_t)pred & (pred_dtype == FV_F32 ? 3 : 1)) == 0 &&
               (table || ((uintptr_t)img & 3) == 0) && ((uintptr_t)table & 15) == 0,
           "%s: a buffer is not aligned to its element size (the table: 16 bytes)", what);
  return FV_OK;
}

Geom geometry(const void* img, bool u8, const void* pred, const void* dpred, int pred_dtype, int batch, int height, int width,
              int patch) {
  Geom G;
  G.H = height; G.W = width; G.p = patch; G.gw = width / patch;
  G.L = (height / patch) * G.gw;
  G.D = 3 * patch * patch;
  G.iv = image_vec(img, u8, width, patch);
  G.pv = pred_vec(pred, dpred, pred_dtype);
  G.rows = (long)batch * G.L;
  return G;
}

size_t lds_bytes(const Geom& G) { return sizeof(float) * (ML_TABLE_FLOATS + (size_t)ML_WAVES * G.D); }

}  // namespace

extern "C" int fv_mae_loss_ok(int batch, int chans, int height, int width, int patch, int pred_dtype) {
  return shape_ok(batch, chans, height, width, patch, pred_dtype) ? 1 : 0;
}

extern "C" int fv_mae_loss_fwd(const void* img, const float* table, const void* pred, int pred_dtype, const float* mask,
                               float* loss_rows, float* row_stats, float* out, int batch, int height, int width, int patch,
                               int norm_pix, fv_stream_t stream) {
  const int rc = check_common("mae_loss_fwd", img, table, pred, pred_dtype, mask, batch, height, width, patch);
  if (rc != FV_OK) return rc;
  FV_CHECK(loss_rows && row_stats && out, "mae_loss_fwd: null pointer");
  FV_CHECK((((uintptr_t)loss_rows | (uintptr_t)row_stats | (uintptr_t)out) & 3) == 0, "mae_loss_fwd: an output is not 4-byte aligned");
  const Geom G = geometry(img, table != nullptr, pred, nullptr, pred_dtype, batch, height, width, patch);
  const dim3 grid(fv_cdiv(G.rows, ML_WAVES)), block(256);
  const size_t smem = lds_bytes(G);
  hipStream_t st = (hipStream_t)stream;
  const float inv_d = 1.f / (float)G.D, inv_dm1 = 1.f / (float)(G.D - 1);
#define FV_ML_ROWS(TP, U8) hipLaunchKernelGGL((mae_loss_rows_kernel<TP, U8>), grid, block, smem, st, img, table, (const TP*)pred, mask, loss_rows, row_stats, G, norm_pix, inv_d, inv_dm1)
  if (pred_dtype == FV_BF16) { if (table) FV_ML_ROWS(bf16_t, true); else FV_ML_ROWS(bf16_t, false); }
  else { if (table) FV_ML_ROWS(float, true); else FV_ML_ROWS(float, false); }
#undef FV_ML_ROWS
  const int vec = (((uintptr_t)loss_rows | (uintptr_t)mask) & 15) == 0;
  hipLaunchKernelGGL(mae_loss_final_kernel, dim3(1), dim3(ML_FINAL_THREADS), 0, st, (const float*)loss_rows, mask, out, G.rows, vec);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_mae_loss_bwd(const void* img, const float* table, const void* pred, int pred_dtype, const float* mask,
                               const float* row_stats, const float* sum_mask, const float* g, void* dpred, int batch, int height,
                               int width, int patch, fv_stream_t stream) {
  const int rc = check_common("mae_loss_bwd", img, table, pred, pred_dtype, mask, batch, height, width, patch);
  if (rc != FV_OK) return rc;
  FV_CHECK(row_stats && sum_mask && g && dpred, "mae_loss_bwd: null pointer");
  FV_CHECK((((uintptr_t)row_stats | (uintptr_t)sum_mask | (uintptr_t)g) & 3) == 0 &&
               ((uintptr_t)dpred & (pred_dtype == FV_F32 ? 3 : 1)) == 0,
           "mae_loss_bwd: a buffer is not aligned to its element size");
  const Geom G = geometry(img, table != nullptr, pred, dpred, pred_dtype, batch, height, width, patch);
  const dim3 grid(fv_cdiv(G.rows, ML_WAVES)), block(256);
  const size_t smem = lds_bytes(G);
  hipStream_t st = (hipStream_t)stream;
  const float two_inv_d = 2.f / (float)G.D;
#define FV_ML_BWD(TP, U8) hipLaunchKernelGGL((mae_loss_bwd_kernel<TP, U8>), grid, block, smem, st, img, table, (const TP*)pred, mask, row_stats, sum_mask, g, (TP*)dpred, G, two_inv_d)
  if (pred_dtype == FV_BF16) { if (table) FV_ML_BWD(bf16_t, true); else FV_ML_BWD(bf16_t, false); }
  else { if (table) FV_ML_BWD(float, true); else FV_ML_BWD(float, false); }
#undef FV_ML_BWD
  FV_LAUNCH_CHECK();
  return FV_OK;
}
