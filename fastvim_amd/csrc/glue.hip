// Small memory-bound ops around the backbone that the training step would otherwise run as strings of library
// elementwise / reduce launches (each a 2.5-5 us node of the captured step):
//   * patch unfold + cast: the k == stride patch-embed Conv2d (models/fastvim.py:95) as a GEMM operand;
//   * batch-mode Mixup / CutMix of the images, on its own and folded into the patch unfold;
//   * the channel models' embed under hierarchical channel sampling: per-channel patch unfold with the channel gather, the
//     per-token table of the patch GEMM's epilogue, the scatter of the channel-embedding gradient rows;
//   * token mean pool and its adjoint (models/fastvim.py:529-531, final_pool_type == "mean");
//   * the stochastic-depth keep table (timm DropPath: floor(keep + U) / keep, one row per DropPath module);
//   * scale-by-a-device-scalar + cast (the loss gradient handed to the head), column sums (head bias gradient).
#include "common.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <typename T> struct Vec4;      // four consecutive elements <-> four floats
template <> struct Vec4<float> {
  static __device__ __forceinline__ void ld(const float* p, float (&v)[4]) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
  static __device__ __forceinline__ void st(float* p, const float (&v)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
};
template <> struct Vec4<bf16_t> {
  static __device__ __forceinline__ void ld(const bf16_t* p, float (&v)[4]) {
    const u32x2 t = *reinterpret_cast<const u32x2*>(p);
    v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xffff0000u);
    v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xffff0000u);
  }
  static __device__ __forceinline__ void st(bf16_t* p, const float (&v)[4]) {
    u32x2 t;
    t.x = pack_bf16x2(v[0], v[1]);
    t.y = pack_bf16x2(v[2], v[3]);
    *reinterpret_cast<u32x2*>(p) = t;
  }
};

// ---- patch unfold: out[b][gi*gw + gj][(c*ph + pi)*pw + pj] = img[b][c][gi*ph + pi][gj*pw + pj] ------------------
// One workgroup per (chunk of GJ patches, patch row, image): image rows come in as 16-byte segments (coalesced along
// W), are converted and placed at their position inside the patch row in LDS; the GJ patch rows are one contiguous
// stretch of `out` and leave as 16-byte stores.
constexpr int UNF_GJ = 16;

template <typename TI, typename TO>
__global__ __launch_bounds__(256) void patch_unfold_kernel(const TI* __restrict__ img, TO* __restrict__ out, int C, int H,
                                                           int W, int ph, int pw, int gw) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  TO* tile = reinterpret_cast<TO*>(smem);
  const int gj0 = blockIdx.x * UNF_GJ, gi = blockIdx.y, b = blockIdx.z;
  const int gjn = min(UNF_GJ, gw - gj0);
  const int Kp = C * ph * pw;                 // elements per patch row
  const int xv = gjn * pw / 4;                // 4-element vectors per image-row segment of the chunk
  const TI* src = img + ((size_t)b * C * H + (size_t)gi * ph) * W + (size_t)gj0 * pw;
  for (int e = threadIdx.x; e < C * ph * xv; e += blockDim.x) {
    const int row = e / xv, x = (e - row * xv) * 4;      // row = c * ph + pi
    const int c = row / ph, pi = row - c * ph;
    float v[4];
    Vec4<TI>::ld(src + ((size_t)c * H + pi) * W + x, v);
    const int gj = x / pw, pj = x - gj * pw;
    Vec4<TO>::st(tile + (size_t)gj * Kp + row * pw + pj, v);
  }
  __syncthreads();
  TO* dst = out + (((size_t)b * gridDim.y + gi) * gw + gj0) * Kp;
  constexpr int EV = 16 / sizeof(TO);
  const int nv = gjn * Kp / EV;
  for (int e = threadIdx.x; e < nv; e += blockDim.x)
    reinterpret_cast<u32x4*>(dst)[e] = reinterpret_cast<const u32x4*>(tile)[e];
}

// ---- per-channel patch unfold with a channel gather (hierarchical channel sampling of the channel models) --------------
//   out[b][(p*n + k)][pi*pw + pj] = img[b][sel[k]][gi*ph + pi][gj*pw + pj],  p = gi*gw + gj  (COLWISE: gj*gh + gi)
// patch_unfold_kernel with the channel looked up in `sel` (device memory, read when the kernel runs; NULL: identity) and
// `gjc` patches per workgroup chosen by the host (n * ph * pw elements per patch must fit the tile).  Rowwise the gjc
// patches are one contiguous stretch of `out`; colwise each patch's n*ph*pw elements are one.  An index outside
// [0, Ctot) is clamped: a block that was never written must not make the kernel read outside the image.
__device__ __forceinline__ int sel_channel(const int32_t* __restrict__ sel, int k, int Ctot) {
  return sel ? min(max(sel[k], 0), Ctot - 1) : k;
}

template <typename TI, typename TO, bool COLWISE>
__global__ __launch_bounds__(256) void patch_unfold_chan_kernel(const TI* __restrict__ img, TO* __restrict__ out,
                                                                const int32_t* __restrict__ sel, int n, int Ctot, int H, int W,
                                                                int ph, int pw, int gw, int gjc) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  TO* tile = reinterpret_cast<TO*>(smem);
  const int gj0 = blockIdx.x * gjc, gi = blockIdx.y, b = blockIdx.z, gh = gridDim.y;
  const int gjn = min(gjc, gw - gj0);
  const int Kp = n * ph * pw;                 // elements per patch position
  const int xv = gjn * pw / 4;                // 4-element vectors per image-row segment of the chunk
  const TI* src = img + ((size_t)b * Ctot * H + (size_t)gi * ph) * W + (size_t)gj0 * pw;
  for (int e = threadIdx.x; e < n * ph * xv; e += blockDim.x) {
    const int row = e / xv, x = (e - row * xv) * 4;      // row = k * ph + pi
    const int k = row / ph, pi = row - k * ph;
    float v[4];
    Vec4<TI>::ld(src + ((size_t)sel_channel(sel, k, Ctot) * H + pi) * W + x, v);
    const int gj = x / pw, pj = x - gj * pw;
    Vec4<TO>::st(tile + (size_t)gj * Kp + row * pw + pj, v);
  }
  __syncthreads();
  constexpr int EV = 16 / sizeof(TO);
  if constexpr (!COLWISE) {
    TO* dst = out + (((size_t)b * gh + gi) * gw + gj0) * Kp;
    const int nv = gjn * Kp / EV;
    for (int e = threadIdx.x; e < nv; e += blockDim.x)
      reinterpret_cast<u32x4*>(dst)[e] = reinterpret_cast<const u32x4*>(tile)[e];
  } else {
    const int pv = Kp / EV;                   // 16-byte vectors per patch position (pw % 8 == 0)
    for (int e = threadIdx.x; e < gjn * pv; e += blockDim.x) {
      const int gj = e / pv, r = e - gj * pv;
      TO* dst = out + (((size_t)b * gw + gj0 + gj) * gh + gi) * Kp;
      reinterpret_cast<u32x4*>(dst)[r] = reinterpret_cast<const u32x4*>(tile)[e];
    }
  }
}

// table[(p*n + k)][d] = (chan[sel[k]][d] + bias[d]) + pos[p][d] in fp32, the sums in this association (what the eager
// epilogue of PatchEmbedPerChannel computes term by term); bias / pos may be absent.
__global__ __launch_bounds__(256) void chan_embed_table_kernel(const float* __restrict__ chan, const float* __restrict__ bias,
                                                               const float* __restrict__ pos, float* __restrict__ table,
                                                               const int32_t* __restrict__ sel, int n, int Ctot, int D, size_t total) {
#pragma clang fp reassociate(off) contract(off)
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int d = (int)(i % D);
    const size_t t = i / D;                   // token = p * n + k
    const int k = (int)(t % n);
    const size_t p = t / n;
    float v = chan[(size_t)sel_channel(sel, k, Ctot) * D + d];
    if (bias) v = v + bias[d];
    if (pos) v = v + pos[p * D + d];
    table[i] = v;
  }
}

// d_table[sel[k]][d] += d_chan[k][d]: the indices of a subset are distinct, so an element of d_table has one owner.
__global__ __launch_bounds__(256) void chan_embed_scatter_kernel(const float* __restrict__ d_chan, float* __restrict__ d_table,
                                                                 const int32_t* __restrict__ sel, int n, int Ctot, int D) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * D) return;
  const int k = i / D, d = i - k * D;
  const int c = sel ? sel[k] : k;
  if (c < 0 || c >= Ctot) return;
  d_table[(size_t)c * D + d] += d_chan[i];
}

// ---- batch-mode Mixup / CutMix (timm.data.Mixup, mode='batch'): image b is mixed with image B-1-b --------------------
// The parameters come from the mix-parameter block in device memory (fv_mix_params, include/fastvim_hip.h), never from a
// launch argument: the host rewrites the block between replays of a captured launch.
template <typename T> __device__ __forceinline__ float round_as(float v);      // v rounded to the storage type T
template <> __device__ __forceinline__ float round_as<float>(float v) {
  asm("" : "+v"(v));          // an opaque copy: the product that made it cannot be contracted into the sum that uses it
  return v;
}
template <> __device__ __forceinline__ float round_as<bf16_t>(float v) { return bf16_bits_to_f32(f32_to_bf16_bits(v)); }

enum { MIX_COPY = 0, MIX_MIXUP = 1, MIX_CUTMIX = 2 };
__device__ __forceinline__ int mix_mode(const fv_mix_params& P) {
  return P.use_cutmix ? MIX_CUTMIX : (P.lam == 1.f ? MIX_COPY : MIX_MIXUP);
}

// Pixels a (image b) and p (image B-1-b) at row y, columns x0 .. x0 + N - 1 -> the mixed pixels of both images.
// Mixup is torch's x.mul(lam).add_(x.flip(0).mul_(1. - lam)) in the storage type T: each product rounded, then the sum
// rounded (-ffast-math would contract one product into the add: 24 % of the pixels change).
template <typename T, int N>
__device__ __forceinline__ void mix_pixels(const fv_mix_params& P, int mode, int y, int x0, const float (&a)[N], const float (&p)[N],
                                           float (&oa)[N], float (&op)[N]) {
#pragma clang fp reassociate(off) contract(off)
  if (mode == MIX_MIXUP) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
      oa[k] = round_as<T>(round_as<T>(a[k] * P.lam) + round_as<T>(p[k] * P.one_minus_lam));
      op[k] = round_as<T>(round_as<T>(p[k] * P.lam) + round_as<T>(a[k] * P.one_minus_lam));
    }
  } else {
    const bool in_rows = mode == MIX_CUTMIX && y >= P.yl && y < P.yh;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const bool in_box = in_rows && x0 + k >= P.xl && x0 + k < P.xh;
      oa[k] = in_box ? p[k] : a[k];
      op[k] = in_box ? a[k] : p[k];
    }
  }
}

// Stand-alone: a thread handles the same position of both images of a pair (two loads, two stores), so the batch is read
// once and written once.  EV = 4: Vec4 accesses (W % 4 == 0 keeps a vector inside an image row); EV = 1: any shape.
template <typename T, int EV>
__global__ __launch_bounds__(256) void mix_batch_kernel(const T* __restrict__ x, T* __restrict__ out,
                                                        const fv_mix_params* __restrict__ mp, int B, int n, int H, int W) {
  const fv_mix_params P = *mp;
  const int mode = mix_mode(P);
  const size_t oa_ = (size_t)blockIdx.y * n, op_ = (size_t)(B - 1 - blockIdx.y) * n;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n / EV; e += gridDim.x * blockDim.x) {
    const int i = e * EV, row = i / W;
    float a[EV], p[EV], ra[EV], rp[EV];
    if constexpr (EV == 4) {
      Vec4<T>::ld(x + oa_ + i, a);
      Vec4<T>::ld(x + op_ + i, p);
    } else {
      a[0] = io<T>::ld(x + oa_ + i);
      p[0] = io<T>::ld(x + op_ + i);
    }
    mix_pixels<T, EV>(P, mode, row % H, i - row * W, a, p, ra, rp);
    if constexpr (EV == 4) {
      Vec4<T>::st(out + oa_ + i, ra);
      Vec4<T>::st(out + op_ + i, rp);
    } else {
      io<T>::st(out + oa_ + i, ra[0]);
      io<T>::st(out + op_ + i, rp[0]);
    }
  }
}

// patch_unfold_kernel over the two images of a pair at once: the same chunk of `gjc` patches of patch row gi of image
// b = blockIdx.z and of image B-1-b.  Every input byte is read once, mixed in registers (in the image's type, as
// mix_batch_kernel mixes it), converted once and placed in the image's own LDS tile; the two tiles leave as 16-byte stores.
template <typename TI, typename TO>
__global__ __launch_bounds__(1024) void patch_unfold_mix_kernel(const TI* __restrict__ img, TO* __restrict__ out,
                                                               const fv_mix_params* __restrict__ mp, int B, int C, int H, int W,
                                                               int ph, int pw, int gw, int gjc) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const fv_mix_params P = *mp;
  const int mode = mix_mode(P);
  const int gj0 = blockIdx.x * gjc, gi = blockIdx.y, ba = blockIdx.z, bp = B - 1 - ba;
  const int gjn = min(gjc, gw - gj0);
  const int Kp = C * ph * pw;                 // elements per patch row
  const int xv = gjn * pw / 4;                // 4-element vectors per image-row segment of the chunk
  TO* tile_a = reinterpret_cast<TO*>(smem);
  TO* tile_p = tile_a + (size_t)gjc * Kp;
  const size_t org = (size_t)gi * ph * W + (size_t)gj0 * pw;
  const TI* src_a = img + (size_t)ba * C * H * W + org;
  const TI* src_p = img + (size_t)bp * C * H * W + org;
  for (int e = threadIdx.x; e < C * ph * xv; e += blockDim.x) {
    const int row = e / xv, x = (e - row * xv) * 4;      // row = c * ph + pi
    const int c = row / ph, pi = row - c * ph;
    const size_t off = ((size_t)c * H + pi) * W + x;
    float a[4], p[4], ra[4], rp[4];
    Vec4<TI>::ld(src_a + off, a);
    Vec4<TI>::ld(src_p + off, p);
    mix_pixels<TI, 4>(P, mode, gi * ph + pi, gj0 * pw + x, a, p, ra, rp);
    const int gj = x / pw, pj = x - gj * pw;
    const size_t t = (size_t)gj * Kp + row * pw + pj;
    Vec4<TO>::st(tile_a + t, ra);
    Vec4<TO>::st(tile_p + t, rp);
  }
  __syncthreads();
  const size_t chunk = ((size_t)gi * gw + gj0) * Kp, image = (size_t)gridDim.y * gw * Kp;
  TO* dst_a = out + (size_t)ba * image + chunk;
  TO* dst_p = out + (size_t)bp * image + chunk;
  constexpr int EV = 16 / sizeof(TO);
  const int nv = gjn * Kp / EV;
  for (int e = threadIdx.x; e < nv; e += blockDim.x) {
    reinterpret_cast<u32x4*>(dst_a)[e] = reinterpret_cast<const u32x4*>(tile_a)[e];
    reinterpret_cast<u32x4*>(dst_p)[e] = reinterpret_cast<const u32x4*>(tile_p)[e];
  }
}

// ---- patch unfold, any even patch width from 8 up (patch 14: FastVim-H, MAE-H) ----------------------------------------
// The kernels above need pw % 8 == 0: a 4-element vector of an image row stays inside one patch and every patch row is a
// 16-byte multiple.  With pw = 14 a 4-element vector straddles a patch boundary every other time (14 % 4 = 2), so it is
// placed into the tile as two 2-element halves (pw even: a pair never straddles).  LV = 4 needs W % 4 == 0 (every image
// row and every chunk's segment then start and end on whole vectors); LV = 2 serves any even W.  The chunk of patches is
// still one contiguous stretch of `out`, but it starts on a 16-byte boundary only for some grids (588 bf16 elements per
// patch are 8-byte multiples; 16 patches are 16-byte ones): `sw`, the bytes per tile store (16, 8 or 4), is the host's
// choice from the actual chunk starts and lengths.
template <typename T> struct Vec2;      // two consecutive elements <-> two floats
template <> struct Vec2<float> {
  static __device__ __forceinline__ void ld(const float* p, float (&v)[2]) {
    const float2 t = *reinterpret_cast<const float2*>(p);
    v[0] = t.x; v[1] = t.y;
  }
  static __device__ __forceinline__ void st(float* p, float a, float b) { *reinterpret_cast<float2*>(p) = make_float2(a, b); }
};
template <> struct Vec2<bf16_t> {
  static __device__ __forceinline__ void ld(const bf16_t* p, float (&v)[2]) {
    const uint32_t t = *reinterpret_cast<const uint32_t*>(p);
    v[0] = __uint_as_float(t << 16); v[1] = __uint_as_float(t & 0xffff0000u);
  }
  static __device__ __forceinline__ void st(bf16_t* p, float a, float b) { *reinterpret_cast<uint32_t*>(p) = pack_bf16x2(a, b); }
};
template <typename T, int LV> __device__ __forceinline__ void ld_row(const T* p, float (&v)[LV]) {
  if constexpr (LV == 4) Vec4<T>::ld(p, v); else Vec2<T>::ld(p, v);
}

// LV elements of row `row` (= c * ph + pi) at column x of the chunk's image-row segment -> their patches' tile rows
template <typename TO, int LV>
__device__ __forceinline__ void place_pairs(TO* tile, int Kp, int pw, int row, int x, const float (&v)[LV]) {
#pragma unroll
  for (int h = 0; h < LV; h += 2) {
    const int gj = (x + h) / pw, pj = (x + h) - gj * pw;
    Vec2<TO>::st(tile + (size_t)gj * Kp + row * pw + pj, v[h], v[h + 1]);
  }
}

// n elements (a multiple of sw bytes, dst sw-byte aligned) from the tile to `out`
template <typename TO>
__device__ __forceinline__ void drain_tile(TO* dst, const TO* tile, int n, int sw) {
  const int nb = n * (int)sizeof(TO);
  if (sw == 16) {
    for (int e = threadIdx.x; e < nb / 16; e += blockDim.x) reinterpret_cast<u32x4*>(dst)[e] = reinterpret_cast<const u32x4*>(tile)[e];
  } else if (sw == 8) {
    for (int e = threadIdx.x; e < nb / 8; e += blockDim.x) reinterpret_cast<u32x2*>(dst)[e] = reinterpret_cast<const u32x2*>(tile)[e];
  } else {
    for (int e = threadIdx.x; e < nb / 4; e += blockDim.x) reinterpret_cast<uint32_t*>(dst)[e] = reinterpret_cast<const uint32_t*>(tile)[e];
  }
}

template <typename TI, typename TO, int LV>
__global__ __launch_bounds__(256) void patch_unfold_even_kernel(const TI* __restrict__ img, TO* __restrict__ out, int C, int H,
                                                                int W, int ph, int pw, int gw, int sw) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  TO* tile = reinterpret_cast<TO*>(smem);
  const int gj0 = blockIdx.x * UNF_GJ, gi = blockIdx.y, b = blockIdx.z;
  const int gjn = min(UNF_GJ, gw - gj0);
  const int Kp = C * ph * pw;                 // elements per patch row
  const int xv = gjn * pw / LV;               // LV-element vectors per image-row segment of the chunk
  const TI* src = img + ((size_t)b * C * H + (size_t)gi * ph) * W + (size_t)gj0 * pw;
  for (int e = threadIdx.x; e < C * ph * xv; e += blockDim.x) {
    const int row = e / xv, x = (e - row * xv) * LV;     // row = c * ph + pi
    const int c = row / ph, pi = row - c * ph;
    float v[LV];
    ld_row<TI, LV>(src + ((size_t)c * H + pi) * W + x, v);
    place_pairs<TO, LV>(tile, Kp, pw, row, x, v);
  }
  __syncthreads();
  drain_tile<TO>(out + (((size_t)b * gridDim.y + gi) * gw + gj0) * Kp, tile, gjn * Kp, sw);
}

// patch_unfold_mix_kernel for any even patch width: the same mixing expressions on the same operands, LV pixels at a time
template <typename TI, typename TO, int LV>
__global__ __launch_bounds__(1024) void patch_unfold_mix_even_kernel(const TI* __restrict__ img, TO* __restrict__ out,
                                                                    const fv_mix_params* __restrict__ mp, int B, int C, int H,
                                                                    int W, int ph, int pw, int gw, int gjc, int sw) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const fv_mix_params P = *mp;
  const int mode = mix_mode(P);
  const int gj0 = blockIdx.x * gjc, gi = blockIdx.y, ba = blockIdx.z, bp = B - 1 - ba;
  const int gjn = min(gjc, gw - gj0);
  const int Kp = C * ph * pw;                 // elements per patch row
  const int xv = gjn * pw / LV;               // LV-element vectors per image-row segment of the chunk
  TO* tile_a = reinterpret_cast<TO*>(smem);
  TO* tile_p = tile_a + (size_t)gjc * Kp;
  const size_t org = (size_t)gi * ph * W + (size_t)gj0 * pw;
  const TI* src_a = img + (size_t)ba * C * H * W + org;
  const TI* src_p = img + (size_t)bp * C * H * W + org;
  for (int e = threadIdx.x; e < C * ph * xv; e += blockDim.x) {
    const int row = e / xv, x = (e - row * xv) * LV;     // row = c * ph + pi
    const int c = row / ph, pi = row - c * ph;
    const size_t off = ((size_t)c * H + pi) * W + x;
    float a[LV], p[LV], ra[LV], rp[LV];
    ld_row<TI, LV>(src_a + off, a);
    ld_row<TI, LV>(src_p + off, p);
    mix_pixels<TI, LV>(P, mode, gi * ph + pi, gj0 * pw + x, a, p, ra, rp);
    place_pairs<TO, LV>(tile_a, Kp, pw, row, x, ra);
    place_pairs<TO, LV>(tile_p, Kp, pw, row, x, rp);
  }
  __syncthreads();
  const size_t chunk = ((size_t)gi * gw + gj0) * Kp, image = (size_t)gridDim.y * gw * Kp;
  drain_tile<TO>(out + (size_t)ba * image + chunk, tile_a, gjn * Kp, sw);
  drain_tile<TO>(out + (size_t)bp * image + chunk, tile_p, gjn * Kp, sw);
}

// ---- token mean pool: out[b][d] = (1/L) sum_l x[b][l][d] ------------------------------------------------------------
// One 16-wave workgroup per (batch element, 4*64-channel slab): lane = 4 channels, the waves split the tokens (four
// loads in flight each -- with 4 waves and one load in flight the 196-token sum was 49 dependent round trips, 15 us),
// fixed-order sum through LDS.
constexpr int MP_WAVES = 16;
template <typename T>
__global__ __launch_bounds__(64 * MP_WAVES) void mean_pool_fwd_kernel(const T* __restrict__ x, T* __restrict__ out, int L, int D, float inv) {
  __shared__ float s_acc[MP_WAVES][256];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int d = (blockIdx.x * 64 + lane) * 4, b = blockIdx.y;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  if (d < D) {
    const T* xp = x + (size_t)b * L * D + d;
    int l = wv;
    for (; l + 3 * MP_WAVES < L; l += 4 * MP_WAVES) {
      float v[4][4];
#pragma unroll
      for (int u = 0; u < 4; ++u) Vec4<T>::ld(xp + (size_t)(l + u * MP_WAVES) * D, v[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] += v[u][k];
    }
    for (; l < L; l += MP_WAVES) {
      float v[4];
      Vec4<T>::ld(xp + (size_t)l * D, v);
#pragma unroll
      for (int k = 0; k < 4; ++k) a[k] += v[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) s_acc[wv][lane * 4 + k] = a[k];
  __syncthreads();
  if (wv == 0 && d < D) {
    float r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < MP_WAVES; ++w) t += s_acc[w][lane * 4 + k];
      r[k] = t * inv;
    }
    Vec4<T>::st(out + (size_t)b * D + d, r);
  }
}

// dx[b][l][d] = g[b][d] * (1/L): the product is formed in fp32 and rounded once, as the library's expand / div does
// (inv = 1/L comes from the host: under -ffast-math a device-side 1.f / L is the approximate reciprocal)
template <typename T>
__global__ __launch_bounds__(256) void mean_pool_bwd_kernel(const T* __restrict__ g, T* __restrict__ dx, int L, int D,
                                                            int rows_per_block, float inv) {
  const int b = blockIdx.y, dv = D / 4;
  const int l0 = blockIdx.x * rows_per_block, l1 = min(L, l0 + rows_per_block);
  for (int e = threadIdx.x; e < (l1 - l0) * dv; e += blockDim.x) {
    const int l = l0 + e / dv, d = (e % dv) * 4;
    float v[4];
    Vec4<T>::ld(g + (size_t)b * D + d, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] *= inv;
    Vec4<T>::st(dx + ((size_t)b * L + l) * D + d, v);
  }
}

__global__ __launch_bounds__(256) void droppath_table_kernel(float* __restrict__ table, const float* __restrict__ keep,
                                                             const float* __restrict__ inv, int mods, int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < mods * batch) {
    const int m = i / batch;
    table[i] = floorf(table[i] + keep[m]) * inv[m];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void scale_cast_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                         T* __restrict__ y, size_t n) {
  const float s = scale[0];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    io<T>::st(y + i, x[i] * s);
}

// out[c] (+)= sum_r x[r][c]: lane = column, the 4 waves of a workgroup split the rows, fixed-order sum through LDS
template <typename T>
__global__ __launch_bounds__(256) void column_sum_kernel(const T* __restrict__ x, float* __restrict__ out, int rows, int cols,
                                                         int accumulate) {
  __shared__ float s_acc[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = blockIdx.x * 64 + lane;
  float a = 0.f;
  if (c < cols)
    for (int r = wv; r < rows; r += 4) a += io<T>::ld(x + (size_t)r * cols + c);
  s_acc[wv][lane] = a;
  __syncthreads();
  if (wv == 0 && c < cols) {
    const float t = (s_acc[0][lane] + s_acc[1][lane]) + (s_acc[2][lane] + s_acc[3][lane]);
    out[c] = accumulate ? out[c] + t : t;
  }
}

bool dt_ok(int dt) { return dt == FV_F32 || dt == FV_BF16; }


// Transposed bf16 shadows of up to 64 equal-shape weights in one launch: dst[j] (cols, rows) = src[j] (rows, cols)^T,
// 32 x 32 tiles through LDS (both sides coalesced).  in_proj.weight (2 d_inner, d_model) -> (d_model, 2 d_inner): the
// K-contiguous operand fv_mixer_conv_pool_bwd_dgrad streams into MFMA registers.
constexpr int TRJ_MAX = 64;
struct TransposeJobs {
  const uint16_t* src[TRJ_MAX];
  uint16_t* dst[TRJ_MAX];
  int rows, cols;
};
__global__ __launch_bounds__(256) void transpose_bf16_kernel(TransposeJobs J) {
  __shared__ uint16_t t[32][33];
  const uint16_t* src = J.src[blockIdx.z];
  uint16_t* dst = J.dst[blockIdx.z];
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + ty + 8 * i, c = c0 + tx;
    t[ty + 8 * i][tx] = (r < J.rows && c < J.cols) ? src[(size_t)r * J.cols + c] : (uint16_t)0;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + ty + 8 * i, r = r0 + tx;
    if (r < J.rows && c < J.cols) dst[(size_t)c * J.rows + r] = t[tx][ty + 8 * i];
  }
}


// Fragment-major copies of up to 64 weights (192, K), K-contiguous, in one launch: the 16-byte unit
//   u = ((wv * K / 32 + ks) * 3 + nb) * 64 + lane   holds   src[48 wv + 16 nb + (lane & 15)][32 ks + 8 (lane >> 4) .. + 8)
// -- the MFMA operand lane `lane` of wave wv loads for column block nb at k step ks in fv_mixer_conv_pool_bwd_dgrad_pk
// (K = 768) and fv_mixer_combine_out_proj_addnorm_pk (K = 384); fastvim_amd.mixer_ops.pack_index is the same map.  A thread
// moves one unit: the writes are contiguous, the reads half lines of 16 rows.
constexpr int PKW_ROWS = 192;
struct PackJobs {
  const uint4* src[TRJ_MAX];
  uint4* dst[TRJ_MAX];
  int ks_n;      // K / 32
};
__global__ __launch_bounds__(256) void pack_weight_frags_kernel(PackJobs J) {
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= PKW_ROWS * J.ks_n * 4) return;
  const int lane = u & 63, t = u >> 6, nb = t % 3, ks = (t / 3) % J.ks_n, wv = t / (3 * J.ks_n);
  const int row = 48 * wv + 16 * nb + (lane & 15), unit_in_row = 4 * ks + (lane >> 4);
  J.dst[blockIdx.y][u] = J.src[blockIdx.y][row * (J.ks_n * 4) + unit_in_row];
}

// Fragment-major copies of up to 64 weights (192, 384) for the product in which the weight's ROWS are k (out_proj.weight as
// the operand of its data gradient, phase 4 of fv_mixer_conv_pool_bwd_dgrad_pk2): the 16-byte unit
//   u = ((wv * 6 + ks) * 6 + nb) * 64 + lane   holds   src[32 ks + 8 (lane >> 4) + j][96 wv + 16 nb + (lane & 15)], j = 0..7
// (fastvim_amd.mixer_ops.pack_index_w2 is the same map).  A thread moves one unit: the writes are contiguous, the reads
// gather 8 rows at a 768-byte stride straight from the plain shadow.
constexpr int PKW2_N = 384, PKW2_UNITS = PKW_ROWS * PKW2_N / 8;
struct PackJobsW2 {
  const uint16_t* src[TRJ_MAX];
  uint4* dst[TRJ_MAX];
};
__global__ __launch_bounds__(256) void pack_weight_frags_w2_kernel(PackJobsW2 J) {
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= PKW2_UNITS) return;
  const int lane = u & 63, t = u >> 6, nb = t % 6, ks = (t / 6) % 6, wv = t / 36;
  const uint16_t* s = J.src[blockIdx.y] + (32 * ks + 8 * (lane >> 4)) * PKW2_N + 96 * wv + 16 * nb + (lane & 15);
  uint32_t w[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = (uint32_t)s[(2 * j) * PKW2_N] | ((uint32_t)s[(2 * j + 1) * PKW2_N] << 16);
  J.dst[blockIdx.y][u] = make_uint4(w[0], w[1], w[2], w[3]);
}

// Fragment-major copies of up to 64 weights (N, 192), K-contiguous, N a multiple of 384, for the forward product in which the
// weight's rows are output columns dealt 96 per wave and 384 per pass (in_proj.weight in fv_gemm_bf16_inproj_pk): the
// 16-byte unit
//   u = (((p * 4 + wv) * 6 + ks) * 6 + nb) * 64 + lane   holds   src[384 p + 96 wv + 16 nb + (lane & 15)][32 ks + 8 (lane >> 4) .. + 8)
// (fastvim_amd.mixer_ops.pack_index_in is the same map).  A thread moves one unit: the writes are contiguous, the reads
// 16-byte pieces of 16 rows.
constexpr int PKIN_K = 192;
struct PackJobsIn {
  const uint4* src[TRJ_MAX];
  uint4* dst[TRJ_MAX];
  int units;     // N * 192 / 8
};
__global__ __launch_bounds__(256) void pack_weight_frags_in_kernel(PackJobsIn J) {
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= J.units) return;
  const int lane = u & 63, t = u >> 6, nb = t % 6, ks = (t / 6) % 6, wv = (t / 36) & 3, p = t / 144;
  const int row = 384 * p + 96 * wv + 16 * nb + (lane & 15), unit_in_row = 4 * ks + (lane >> 4);
  J.dst[blockIdx.y][u] = J.src[blockIdx.y][row * (PKIN_K / 8) + unit_in_row];
}

// Bytes per tile store of the even-width unfold forms.  Chunks of `gjc` patches start at patch (b*gh + gi)*gw + k*gjc and
// hold gjc or gw - k*gjc patches: every start and length is a multiple of gcd(gw, gjc) patches of `patch_bytes` each
// (a multiple of 4: the width is even, an element at least 2 bytes), and `out` itself is 16-byte aligned.
int unfold_store_bytes(int gw, int gjc, size_t patch_bytes) {
  int a = gw, b = gjc;
  while (b) { const int t = a % b; a = b; b = t; }
  const size_t unit = (size_t)a * patch_bytes;
  return unit % 16 == 0 ? 16 : unit % 8 == 0 ? 8 : 4;
}

}  // namespace

extern "C" int fv_patch_unfold(const void* img, int img_dtype, void* out, int out_dtype, int batch, int chans, int height,
                               int width, int ph, int pw, fv_stream_t stream) {
  FV_CHECK(img && out, "patch_unfold: null pointer");
  FV_CHECK(dt_ok(img_dtype) && dt_ok(out_dtype), "patch_unfold: dtypes must be fp32 or bf16");
  FV_CHECK(batch > 0 && chans > 0 && ph > 0 && pw > 0 && height >= ph && width >= pw, "patch_unfold: empty dimension");
  FV_CHECK(height % ph == 0 && width % pw == 0, "patch_unfold: image %dx%d is not whole %dx%d patches", height, width, ph, pw);
  FV_CHECK(pw % 2 == 0 && pw >= 8 && ((uintptr_t)img & 15) == 0 && ((uintptr_t)out & 15) == 0,
           "patch_unfold: patch width must be even and at least 8, and the buffers 16-byte aligned");
  const int gh = height / ph, gw = width / pw;
  const size_t osz = out_dtype == FV_F32 ? 4 : 2;
  const size_t smem = (size_t)UNF_GJ * chans * ph * pw * osz;
  FV_CHECK(smem <= 64 * 1024, "patch_unfold: %d x %d x %d patches do not fit the staging tile", chans, ph, pw);
  FV_CHECK(gh <= 65535 && batch <= 65535, "patch_unfold: grid too large");
  const dim3 grid(fv_cdiv(gw, UNF_GJ), gh, batch), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (pw % 8 != 0) {
    const int sw = unfold_store_bytes(gw, UNF_GJ, (size_t)chans * ph * pw * osz);
#define FV_UNFE(TI, TO) do { if (width % 4 == 0) hipLaunchKernelGGL((patch_unfold_even_kernel<TI, TO, 4>), grid, block, smem, st, (const TI*)img, (TO*)out, chans, height, width, ph, pw, gw, sw); \
                             else hipLaunchKernelGGL((patch_unfold_even_kernel<TI, TO, 2>), grid, block, smem, st, (const TI*)img, (TO*)out, chans, height, width, ph, pw, gw, sw); } while (0)
    if (img_dtype == FV_F32 && out_dtype == FV_BF16) FV_UNFE(float, bf16_t);
    else if (img_dtype == FV_F32) FV_UNFE(float, float);
    else if (out_dtype == FV_BF16) FV_UNFE(bf16_t, bf16_t);
    else FV_UNFE(bf16_t, float);
#undef FV_UNFE
    FV_LAUNCH_CHECK();
    return FV_OK;
  }
#define FV_UNF(TI, TO) hipLaunchKernelGGL((patch_unfold_kernel<TI, TO>), grid, block, smem, st, (const TI*)img, (TO*)out, chans, height, width, ph, pw, gw)
  if (img_dtype == FV_F32 && out_dtype == FV_BF16) FV_UNF(float, bf16_t);
  else if (img_dtype == FV_F32) FV_UNF(float, float);
  else if (out_dtype == FV_BF16) FV_UNF(bf16_t, bf16_t);
  else FV_UNF(bf16_t, float);
#undef FV_UNF
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_patch_unfold_chan(const void* img, int img_dtype, void* out, int out_dtype, int batch, int chans_total,
                                    int height, int width, int ph, int pw, const int32_t* sel, int n_sel, int colwise,
                                    fv_stream_t stream) {
  FV_CHECK(img && out, "patch_unfold_chan: null pointer");
  FV_CHECK(dt_ok(img_dtype) && dt_ok(out_dtype), "patch_unfold_chan: dtypes must be fp32 or bf16");
  FV_CHECK(batch > 0 && chans_total > 0 && ph > 0 && pw > 0 && height >= ph && width >= pw, "patch_unfold_chan: empty dimension");
  FV_CHECK(n_sel > 0 && n_sel <= chans_total, "patch_unfold_chan: %d selected channels of %d", n_sel, chans_total);
  FV_CHECK(height % ph == 0 && width % pw == 0, "patch_unfold_chan: image %dx%d is not whole %dx%d patches", height, width, ph, pw);
  FV_CHECK(pw % 8 == 0 && ((uintptr_t)img & 15) == 0 && ((uintptr_t)out & 15) == 0,
           "patch_unfold_chan: patch width must be a multiple of 8 and the buffers 16-byte aligned");
  const int gh = height / ph, gw = width / pw;
  const size_t osz = out_dtype == FV_F32 ? 4 : 2;
  // patches per workgroup: at most UNF_GJ, a tile of at most 32 KB (two workgroups per CU keep loads in flight while
  // one drains its tile), and the patch row cut into equal chunks (14 patches under a limit of 8: 7 + 7, not 8 + 6)
  const size_t per_patch = (size_t)n_sel * ph * pw * osz;
  FV_CHECK(per_patch <= 64 * 1024, "patch_unfold_chan: %d x %d x %d patches do not fit the staging tile", n_sel, ph, pw);
  int fit = (int)((32 * 1024) / per_patch);
  fit = fit < 1 ? 1 : (fit > UNF_GJ ? UNF_GJ : fit);
  const int gjc = fv_cdiv(gw, fv_cdiv(gw, fit));
  const size_t smem = gjc * per_patch;
  FV_CHECK(gh <= 65535 && batch <= 65535, "patch_unfold_chan: grid too large");
  const dim3 grid(fv_cdiv(gw, gjc), gh, batch), block(256);
  hipStream_t st = (hipStream_t)stream;
#define FV_UNFC2(TI, TO, CW) hipLaunchKernelGGL((patch_unfold_chan_kernel<TI, TO, CW>), grid, block, smem, st, (const TI*)img, (TO*)out, sel, n_sel, chans_total, height, width, ph, pw, gw, gjc)
#define FV_UNFC(TI, TO) do { if (colwise) FV_UNFC2(TI, TO, true); else FV_UNFC2(TI, TO, false); } while (0)
  if (img_dtype == FV_F32 && out_dtype == FV_BF16) FV_UNFC(float, bf16_t);
  else if (img_dtype == FV_F32) FV_UNFC(float, float);
  else if (out_dtype == FV_BF16) FV_UNFC(bf16_t, bf16_t);
  else FV_UNFC(bf16_t, float);
#undef FV_UNFC
#undef FV_UNFC2
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_chan_embed_table(const float* chan_table, const float* bias, const float* pos, float* table, const int32_t* sel,
                                   int n_sel, int chans_total, int positions, int dim, fv_stream_t stream) {
  FV_CHECK(chan_table && table, "chan_embed_table: null pointer");
  FV_CHECK(n_sel > 0 && n_sel <= chans_total && positions > 0 && dim > 0, "chan_embed_table: bad shape (%d of %d channels, %d positions, dim %d)",
           n_sel, chans_total, positions, dim);
  const size_t total = (size_t)positions * n_sel * dim;
  const long blocks = fv_cdiv((long)total, 256l);
  hipLaunchKernelGGL(chan_embed_table_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream,
                     chan_table, bias, pos, table, sel, n_sel, chans_total, dim, total);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_chan_embed_scatter(const float* d_chan, float* d_table, const int32_t* sel, int n_sel, int chans_total, int dim,
                                     fv_stream_t stream) {
  FV_CHECK(d_chan && d_table, "chan_embed_scatter: null pointer");
  FV_CHECK(n_sel > 0 && n_sel <= chans_total && dim > 0 && (long)n_sel * dim < (1l << 31), "chan_embed_scatter: bad shape (%d of %d channels, dim %d)",
           n_sel, chans_total, dim);
  hipLaunchKernelGGL(chan_embed_scatter_kernel, dim3(fv_cdiv(n_sel * dim, 256)), dim3(256), 0, (hipStream_t)stream,
                     d_chan, d_table, sel, n_sel, chans_total, dim);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_mix_batch(const void* x, void* out, int dtype, int batch, int chans, int height, int width, const void* mix,
                            fv_stream_t stream) {
  FV_CHECK(x && out && mix && x != out, "mix_batch: null or aliased pointer (the op is out of place)");
  FV_CHECK(dt_ok(dtype), "mix_batch: dtype must be fp32 or bf16");
  FV_CHECK(batch > 0 && chans > 0 && height > 0 && width > 0, "mix_batch: empty dimension");
  FV_CHECK(batch % 2 == 0, "mix_batch: batch mode pairs image b with image batch-1-b, the batch (%d) must be even", batch);
  const long n = (long)chans * height * width;
  FV_CHECK(n < (1l << 31) && batch / 2 <= 65535, "mix_batch: image or batch too large");
  const size_t esz = dtype == FV_F32 ? 4 : 2;
  const bool vec = width % 4 == 0 && ((uintptr_t)x % (4 * esz)) == 0 && ((uintptr_t)out % (4 * esz)) == 0;
  const long work = vec ? n / 4 : n;
  const dim3 grid(fv_cdiv(work, 256) < 1024 ? fv_cdiv(work, 256) : 1024, batch / 2), block(256);
  hipStream_t st = (hipStream_t)stream;
  const fv_mix_params* mp = (const fv_mix_params*)mix;
#define FV_MIXB(T, EV) hipLaunchKernelGGL((mix_batch_kernel<T, EV>), grid, block, 0, st, (const T*)x, (T*)out, mp, batch, (int)n, height, width)
  if (dtype == FV_F32) { if (vec) FV_MIXB(float, 4); else FV_MIXB(float, 1); }
  else { if (vec) FV_MIXB(bf16_t, 4); else FV_MIXB(bf16_t, 1); }
#undef FV_MIXB
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_patch_unfold_mix(const void* img, int img_dtype, void* out, int out_dtype, int batch, int chans, int height,
                                   int width, int ph, int pw, const void* mix, fv_stream_t stream) {
  FV_CHECK(img && out && mix, "patch_unfold_mix: null pointer");
  FV_CHECK(dt_ok(img_dtype) && dt_ok(out_dtype), "patch_unfold_mix: dtypes must be fp32 or bf16");
  FV_CHECK(batch > 0 && chans > 0 && ph > 0 && pw > 0 && height >= ph && width >= pw, "patch_unfold_mix: empty dimension");
  FV_CHECK(batch % 2 == 0, "patch_unfold_mix: batch mode pairs image b with image batch-1-b, the batch (%d) must be even", batch);
  FV_CHECK(height % ph == 0 && width % pw == 0, "patch_unfold_mix: image %dx%d is not whole %dx%d patches", height, width, ph, pw);
  FV_CHECK(pw % 2 == 0 && pw >= 8 && ((uintptr_t)img & 15) == 0 && ((uintptr_t)out & 15) == 0,
           "patch_unfold_mix: patch width must be even and at least 8, and the buffers 16-byte aligned");
  const int gh = height / ph, gw = width / pw;
  const size_t osz = out_dtype == FV_F32 ? 4 : 2;
  // Two tiles per workgroup.  What this kernel is short of is loads in flight per byte of LDS: with fv_patch_unfold's
  // shape (16 patches, 256 threads) the doubled tile halves the workgroups a CU holds, and the launch ran 12 % behind
  // the plain unfold; 8 patches per tile -- the plain kernel's LDS footprint -- under 512 threads runs ahead of it
  // (*Mixup*).  fv_patch_unfold's own limit (16 patches in 64 KB) is then the limit here too.
  const size_t per_patch = 2 * (size_t)chans * ph * pw * osz;
  const int gjc = fv_tune("FASTVIM_UNFOLD_MIX_GJ", UNF_GJ / 2);
  const int threads = fv_tune("FASTVIM_UNFOLD_MIX_THREADS", 512);
  const size_t smem = gjc * per_patch;
  FV_CHECK(gjc > 0 && smem <= 64 * 1024, "patch_unfold_mix: %d x %d x %d patches do not fit the staging tiles", chans, ph, pw);
  FV_CHECK(threads >= 64 && threads <= 1024 && threads % 64 == 0, "patch_unfold_mix: bad workgroup size %d", threads);
  FV_CHECK(gh <= 65535 && batch / 2 <= 65535, "patch_unfold_mix: grid too large");
  const dim3 grid(fv_cdiv(gw, gjc), gh, batch / 2), block(threads);
  hipStream_t st = (hipStream_t)stream;
  const fv_mix_params* mp = (const fv_mix_params*)mix;
  if (pw % 8 != 0) {
    FV_CHECK(gjc % 2 == 0, "patch_unfold_mix: patch width %d needs an even number of patches per tile (got %d)", pw, gjc);
    const int sw = unfold_store_bytes(gw, gjc, (size_t)chans * ph * pw * osz);
#define FV_UNFME(TI, TO) do { if (width % 4 == 0) hipLaunchKernelGGL((patch_unfold_mix_even_kernel<TI, TO, 4>), grid, block, smem, st, (const TI*)img, (TO*)out, mp, batch, chans, height, width, ph, pw, gw, gjc, sw); \
                              else hipLaunchKernelGGL((patch_unfold_mix_even_kernel<TI, TO, 2>), grid, block, smem, st, (const TI*)img, (TO*)out, mp, batch, chans, height, width, ph, pw, gw, gjc, sw); } while (0)
    if (img_dtype == FV_F32 && out_dtype == FV_BF16) FV_UNFME(float, bf16_t);
    else if (img_dtype == FV_F32) FV_UNFME(float, float);
    else if (out_dtype == FV_BF16) FV_UNFME(bf16_t, bf16_t);
    else FV_UNFME(bf16_t, float);
#undef FV_UNFME
    FV_LAUNCH_CHECK();
    return FV_OK;
  }
#define FV_UNFM(TI, TO) hipLaunchKernelGGL((patch_unfold_mix_kernel<TI, TO>), grid, block, smem, st, (const TI*)img, (TO*)out, mp, batch, chans, height, width, ph, pw, gw, gjc)
  if (img_dtype == FV_F32 && out_dtype == FV_BF16) FV_UNFM(float, bf16_t);
  else if (img_dtype == FV_F32) FV_UNFM(float, float);
  else if (out_dtype == FV_BF16) FV_UNFM(bf16_t, bf16_t);
  else FV_UNFM(bf16_t, float);
#undef FV_UNFM
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_mean_pool_fwd(const void* x, void* out, int batch, int tokens, int dim, int dtype, fv_stream_t stream) {
  FV_CHECK(x && out, "mean_pool_fwd: null pointer");
  FV_CHECK(dt_ok(dtype), "mean_pool_fwd: dtype must be fp32 or bf16");
  FV_CHECK(batch > 0 && tokens > 0 && dim > 0 && dim % 4 == 0 && batch <= 65535, "mean_pool_fwd: bad shape (%d, %d, %d)", batch, tokens, dim);
  const dim3 grid(fv_cdiv(dim, 256), batch), block(64 * MP_WAVES);
  hipStream_t st = (hipStream_t)stream;
  const float inv = 1.f / (float)tokens;
  if (dtype == FV_F32) hipLaunchKernelGGL(mean_pool_fwd_kernel<float>, grid, block, 0, st, (const float*)x, (float*)out, tokens, dim, inv);
  else hipLaunchKernelGGL(mean_pool_fwd_kernel<bf16_t>, grid, block, 0, st, (const bf16_t*)x, (bf16_t*)out, tokens, dim, inv);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_mean_pool_bwd(const void* g, void* dx, int batch, int tokens, int dim, int dtype, fv_stream_t stream) {
  FV_CHECK(g && dx, "mean_pool_bwd: null pointer");
  FV_CHECK(dt_ok(dtype), "mean_pool_bwd: dtype must be fp32 or bf16");
  FV_CHECK(batch > 0 && tokens > 0 && dim > 0 && dim % 4 == 0 && batch <= 65535, "mean_pool_bwd: bad shape (%d, %d, %d)", batch, tokens, dim);
  const int rpb = fv_cdiv(tokens, 8);
  const dim3 grid(fv_cdiv(tokens, rpb), batch), block(256);
  hipStream_t st = (hipStream_t)stream;
  const float inv = 1.f / (float)tokens;
  if (dtype == FV_F32) hipLaunchKernelGGL(mean_pool_bwd_kernel<float>, grid, block, 0, st, (const float*)g, (float*)dx, tokens, dim, rpb, inv);
  else hipLaunchKernelGGL(mean_pool_bwd_kernel<bf16_t>, grid, block, 0, st, (const bf16_t*)g, (bf16_t*)dx, tokens, dim, rpb, inv);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_droppath_table(float* table, const float* keep, const float* inv_keep, int mods, int batch, fv_stream_t stream) {
  FV_CHECK(table && keep && inv_keep && mods > 0 && batch > 0, "droppath_table: bad arguments");
  hipLaunchKernelGGL(droppath_table_kernel, dim3(fv_cdiv((long)mods * batch, 256)), dim3(256), 0, (hipStream_t)stream, table, keep,
                     inv_keep, mods, batch);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_scale_cast(const float* x, const float* scale, void* y, int y_dtype, size_t n, fv_stream_t stream) {
  FV_CHECK(x && scale && y && n > 0, "scale_cast: bad arguments");
  FV_CHECK(dt_ok(y_dtype), "scale_cast: output must be fp32 or bf16");
  const dim3 grid(fv_cdiv((long)n, 256) < 2048 ? fv_cdiv((long)n, 256) : 2048), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (y_dtype == FV_F32) hipLaunchKernelGGL(scale_cast_kernel<float>, grid, block, 0, st, x, scale, (float*)y, n);
  else hipLaunchKernelGGL(scale_cast_kernel<bf16_t>, grid, block, 0, st, x, scale, (bf16_t*)y, n);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_column_sum(const void* x, int dtype, float* out, int rows, int cols, int accumulate, fv_stream_t stream) {
  FV_CHECK(x && out && rows > 0 && cols > 0, "column_sum: bad arguments");
  FV_CHECK(dt_ok(dtype), "column_sum: input must be fp32 or bf16");
  const dim3 grid(fv_cdiv(cols, 64)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == FV_F32) hipLaunchKernelGGL(column_sum_kernel<float>, grid, block, 0, st, (const float*)x, out, rows, cols, accumulate);
  else hipLaunchKernelGGL(column_sum_kernel<bf16_t>, grid, block, 0, st, (const bf16_t*)x, out, rows, cols, accumulate);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_transpose_bf16_batched(const void* const* srcs, void* const* dsts, int njobs, int rows, int cols,
                                         fv_stream_t stream) {
  FV_CHECK(srcs && dsts && njobs > 0 && njobs <= TRJ_MAX, "transpose_bf16_batched: 1..%d jobs", TRJ_MAX);
  FV_CHECK(rows > 0 && cols > 0 && fv_cdiv(rows, 32) <= 65535, "transpose_bf16_batched: bad shape (%d, %d)", rows, cols);
  TransposeJobs J{};
  for (int j = 0; j < njobs; ++j) {
    FV_CHECK(srcs[j] && dsts[j], "transpose_bf16_batched: null pointer in job %d", j);
    J.src[j] = (const uint16_t*)srcs[j];
    J.dst[j] = (uint16_t*)dsts[j];
  }
  J.rows = rows; J.cols = cols;
  hipLaunchKernelGGL(transpose_bf16_kernel, dim3(fv_cdiv(cols, 32), fv_cdiv(rows, 32), njobs), dim3(256), 0, (hipStream_t)stream, J);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_pack_weight_frags_batched(const void* const* srcs, void* const* dsts, int njobs, int K, fv_stream_t stream) {
  FV_CHECK(srcs && dsts && njobs > 0 && njobs <= TRJ_MAX, "pack_weight_frags_batched: 1..%d jobs", TRJ_MAX);
  FV_CHECK(K == 384 || K == 768, "pack_weight_frags_batched: K = %d is not a built reduction length (384, 768)", K);
  PackJobs J{};
  for (int j = 0; j < njobs; ++j) {
    FV_CHECK(srcs[j] && dsts[j] && srcs[j] != dsts[j], "pack_weight_frags_batched: null or aliased pointer in job %d", j);
    FV_CHECK(((uintptr_t)srcs[j] & 15) == 0 && ((uintptr_t)dsts[j] & 15) == 0, "pack_weight_frags_batched: job %d is not 16-byte aligned", j);
    J.src[j] = (const uint4*)srcs[j];
    J.dst[j] = (uint4*)dsts[j];
  }
  J.ks_n = K / 32;
  hipLaunchKernelGGL(pack_weight_frags_kernel, dim3(fv_cdiv(PKW_ROWS * J.ks_n * 4, 256), njobs), dim3(256), 0, (hipStream_t)stream, J);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

// dsts[j] = the fragment-major copy of srcs[j] ((192, 384) bf16 row-major, rows = k) that
// fv_mixer_conv_pool_bwd_dgrad_pk2 streams in its second phase
extern "C" int fv_pack_weight_frags_w2_batched(const void* const* srcs, void* const* dsts, int njobs, fv_stream_t stream) {
  FV_CHECK(srcs && dsts && njobs > 0 && njobs <= TRJ_MAX, "pack_weight_frags_w2_batched: 1..%d jobs", TRJ_MAX);
  PackJobsW2 J{};
  for (int j = 0; j < njobs; ++j) {
    FV_CHECK(srcs[j] && dsts[j] && srcs[j] != dsts[j], "pack_weight_frags_w2_batched: null or aliased pointer in job %d", j);
    FV_CHECK(((uintptr_t)srcs[j] & 1) == 0 && ((uintptr_t)dsts[j] & 15) == 0, "pack_weight_frags_w2_batched: job %d is not aligned", j);
    J.src[j] = (const uint16_t*)srcs[j];
    J.dst[j] = (uint4*)dsts[j];
  }
  hipLaunchKernelGGL(pack_weight_frags_w2_kernel, dim3(fv_cdiv(PKW2_UNITS, 256), njobs), dim3(256), 0, (hipStream_t)stream, J);
  FV_LAUNCH_CHECK();
  return FV_OK;
}

// dsts[j] = the fragment-major copy of srcs[j] ((N, 192) bf16 row-major, N a multiple of 384) that fv_gemm_bf16_inproj_pk
// streams
extern "C" int fv_pack_weight_frags_in_batched(const void* const* srcs, void* const* dsts, int njobs, int N, fv_stream_t stream) {
  FV_CHECK(srcs && dsts && njobs > 0 && njobs <= TRJ_MAX, "pack_weight_frags_in_batched: 1..%d jobs", TRJ_MAX);
  FV_CHECK(N > 0 && N % 384 == 0 && N <= (1 << 20), "pack_weight_frags_in_batched: N = %d is not a multiple of 384", N);
  PackJobsIn J{};
  for (int j = 0; j < njobs; ++j) {
    FV_CHECK(srcs[j] && dsts[j] && srcs[j] != dsts[j], "pack_weight_frags_in_batched: null or aliased pointer in job %d", j);
    FV_CHECK(((uintptr_t)srcs[j] & 15) == 0 && ((uintptr_t)dsts[j] & 15) == 0, "pack_weight_frags_in_batched: job %d is not 16-byte aligned", j);
    J.src[j] = (const uint4*)srcs[j];
    J.dst[j] = (uint4*)dsts[j];
  }
  J.units = N * (PKIN_K / 8);
  hipLaunchKernelGGL(pack_weight_frags_in_kernel, dim3(fv_cdiv(J.units, 256), njobs), dim3(256), 0, (hipStream_t)stream, J);
  FV_LAUNCH_CHECK();
  return FV_OK;
}
