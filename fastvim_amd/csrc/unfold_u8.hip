// Patch unfold of 8-bit images with the per-channel normalisation as a table lookup: the three unfold launches of
// glue.hip (plain, Mixup / CutMix over pairs of images, per-channel with the channel gather) for a `const uint8_t*`
// image and a (channels, 256) fp32 table in device memory.
//
// The contract (*uint8 images*): the HOST builds table[c][v] with torch, in the loader's own order
// of operations; a kernel only looks values up -- no arithmetic that -ffast-math could rewrite -- and from the looked-up
// fp32 value on does what the float kernel does (the same mixing expressions, the same rounding to the output type).
// out == fv_patch_unfold*(table[c][img]) bit for bit.
//
// A workgroup copies the table rows it needs into LDS behind its staging tile (1 KB per channel), loads image-row
// segments LV bytes at a time (16 where the row stride, the chunk width and the base address allow, else 8, 4 or 2 -- the
// float kernels choose between 4- and 2-element pieces the same way), looks every byte up and places the values in the
// tile PV at a time (4 where the patch width is a multiple of 4: a group of 4 pixels never straddles a patch; else
// pairs).  The lookup is a ds_read_b32 at a data-dependent address: lanes of a 32-lane half that hit the same bank (32
// banks for this instruction) with DIFFERENT pixel values serialise, equal values broadcast.  fp32 entries are kept --
// one table for both output types and for the mixing expressions, which need the fp32 value; a bf16 copy would put two
// entries in a dword and conflict as often.
//
// The small helpers below (element stores, round_as, the mixing expressions, the channel clamp) restate those of glue.hip,
// which this change leaves untouched; tests/test_unfold_u8_gpu.py holds the two files to bit equality.
//
// Random erasing (the _re entry points): ERASE = true forms of the plain and the pair kernel replace, between the lookup
// and the placement / the mixing, the pixels inside the sample's box by 0 or by the noise of erase_noise.h -- what
// fv_random_erase writes into the normalised fp32 image, bit for bit.  The ERASE = false forms are the code they were,
// but for the box test of mix_pixels_f32.
#include "common.h"
#include "erase_noise.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int U8_GJ = 16;        // patches per workgroup of the plain launch (glue.hip: UNF_GJ)
constexpr int U8_MIX_GJ = 8;     // ... per tile of the pair launch, under 512 threads (glue.hip: fv_patch_unfold_mix)
constexpr int U8_MIX_THREADS = 512;

// PV consecutive values -> PV elements of the tile, rounded as glue.hip's Vec4 / Vec2 stores round them
template <typename TO, int PV> struct StoreV;
template <> struct StoreV<float, 4> {
  static __device__ __forceinline__ void st(float* p, const float* v) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};
template <> struct StoreV<float, 2> {
  static __device__ __forceinline__ void st(float* p, const float* v) { *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]); }
};
template <> struct StoreV<bf16_t, 4> {
  static __device__ __forceinline__ void st(bf16_t* p, const float* v) {
    u32x2 t;
    t.x = pack_bf16x2(v[0], v[1]);
    t.y = pack_bf16x2(v[2], v[3]);
    *reinterpret_cast<u32x2*>(p) = t;
  }
};
template <> struct StoreV<bf16_t, 2> {
  static __device__ __forceinline__ void st(bf16_t* p, const float* v) { *reinterpret_cast<uint32_t*>(p) = pack_bf16x2(v[0], v[1]); }
};

// LV bytes at p (LV-byte aligned) -> their entries of the channel's table row (LDS).  Bytes are UNSIGNED: shifts and
// masks of an unsigned word, never a char.
template <int LV>
__device__ __forceinline__ void lookup_row(const uint8_t* __restrict__ p, const float* __restrict__ trow, float (&v)[LV]) {
  if constexpr (LV == 2) {
    const uint32_t w = *reinterpret_cast<const uint16_t*>(p);
    v[0] = trow[w & 0xffu];
    v[1] = trow[w >> 8];
  } else {
    uint32_t w[LV / 4];
    if constexpr (LV == 16) {
      const u32x4 t = *reinterpret_cast<const u32x4*>(p);
      w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
    } else if constexpr (LV == 8) {
      const u32x2 t = *reinterpret_cast<const u32x2*>(p);
      w[0] = t.x; w[1] = t.y;
    } else {
      w[0] = *reinterpret_cast<const uint32_t*>(p);
    }
#pragma unroll
    for (int j = 0; j < LV; ++j) v[j] = trow[(w[j >> 2] >> (8 * (j & 3))) & 0xffu];
  }
}

// LV values of row `row` (= c * ph + pi) at column x of the chunk's image-row segment -> their patches' tile rows
template <typename TO, int LV, int PV>
__device__ __forceinline__ void place_row(TO* tile, int Kp, int pw, int row, int x, const float (&v)[LV]) {
#pragma unroll
  for (int h = 0; h < LV; h += PV) {
    const int gj = (x + h) / pw, pj = (x + h) - gj * pw;
    StoreV<TO, PV>::st(tile + (size_t)gj * Kp + row * pw + pj, v + h);
  }
}

// nb bytes (a multiple of sw, dst sw-byte aligned) from the tile to `out`
__device__ __forceinline__ void drain_bytes(void* dst, const void* tile, int nb, int sw) {
  if (sw == 16) {
    for (int e = threadIdx.x; e < nb / 16; e += blockDim.x) reinterpret_cast<u32x4*>(dst)[e] = reinterpret_cast<const u32x4*>(tile)[e];
  } else if (sw == 8) {
    for (int e = threadIdx.x; e < nb / 8; e += blockDim.x) reinterpret_cast<u32x2*>(dst)[e] = reinterpret_cast<const u32x2*>(tile)[e];
  } else {
    for (int e = threadIdx.x; e < nb / 4; e += blockDim.x) reinterpret_cast<uint32_t*>(dst)[e] = reinterpret_cast<const uint32_t*>(tile)[e];
  }
}

// rows [0, rows) of the table -> LDS, 16 bytes at a time (a row is 256 floats = 64 vectors)
__device__ __forceinline__ void stage_table(float* tab, const float* __restrict__ table, int rows) {
  for (int e = threadIdx.x; e < rows * 64; e += blockDim.x)
    reinterpret_cast<float4*>(tab)[e] = reinterpret_cast<const float4*>(table)[e];
}

// ---- plain: out[b][gi*gw + gj][(c*ph + pi)*pw + pj] = table[c][img[b][c][gi*ph + pi][gj*pw + pj]] ---------------------
template <typename TO, int LV, int PV, bool ERASE>
__global__ __launch_bounds__(256) void patch_unfold_u8_kernel(const uint8_t* __restrict__ img, const float* __restrict__ table,
                                                              TO* __restrict__ out, int C, int H, int W, int ph, int pw, int gw,
                                                              int sw, int tile_bytes, const int32_t* __restrict__ erase) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  TO* tile = reinterpret_cast<TO*>(smem);
  float* tab = reinterpret_cast<float*>(smem + tile_bytes);
  stage_table(tab, table, C);
  __syncthreads();
  const int gj0 = blockIdx.x * U8_GJ, gi = blockIdx.y, b = blockIdx.z;
  const int gjn = min(U8_GJ, gw - gj0);
  const int Kp = C * ph * pw;                 // elements per patch row
  const int xv = gjn * pw / LV;               // LV-pixel vectors per image-row segment of the chunk
  const uint8_t* src = img + ((size_t)b * C * H + (size_t)gi * ph) * W + (size_t)gj0 * pw;
  fv_erase::Key ek = {};
  fv_erase::Box eb = {};
  if constexpr (ERASE) {
    ek = fv_erase::load_key(erase);
    eb = fv_erase::load_box(erase, b);
  }
  for (int e = threadIdx.x; e < C * ph * xv; e += blockDim.x) {
    const int row = e / xv, x = (e - row * xv) * LV;     // row = c * ph + pi
    const int c = row / ph, pi = row - c * ph;
    float v[LV];
    lookup_row<LV>(src + ((size_t)c * H + pi) * W + x, tab + c * 256, v);
    if constexpr (ERASE) fv_erase::erase_segment<LV>(ek, eb, b, c, gi * ph + pi, gj0 * pw + x, v);      // (gj0 * pw % 16 == 0)
    place_row<TO, LV, PV>(tile, Kp, pw, row, x, v);
  }
  __syncthreads();
  drain_bytes(out + (((size_t)b * gridDim.y + gi) * gw + gj0) * Kp, tile, gjn * Kp * (int)sizeof(TO), sw);
}

// ---- per-channel with the channel gather: LDS row k of the table is table[sel[k]], clamped like glue.hip's sel_channel --
__device__ __forceinline__ int sel_channel_u8(const int32_t* __restrict__ sel, int k, int Ctot) {
  return sel ? min(max(sel[k], 0), Ctot - 1) : k;
}

template <typename TO, int LV, bool COLWISE>
__global__ __launch_bounds__(256) void patch_unfold_chan_u8_kernel(const uint8_t* __restrict__ img, const float* __restrict__ table,
                                                                   TO* __restrict__ out, const int32_t* __restrict__ sel, int n,
                                                                   int Ctot, int H, int W, int ph, int pw, int gw, int gjc,
                                                                   int tile_bytes) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  TO* tile = reinterpret_cast<TO*>(smem);
  float* tab = reinterpret_cast<float*>(smem + tile_bytes);
  for (int e = threadIdx.x; e < n * 64; e += blockDim.x) {
    const int k = e >> 6;
    reinterpret_cast<float4*>(tab)[e] = reinterpret_cast<const float4*>(table + (size_t)sel_channel_u8(sel, k, Ctot) * 256)[e & 63];
  }
  __syncthreads();
  const int gj0 = blockIdx.x * gjc, gi = blockIdx.y, b = blockIdx.z, gh = gridDim.y;
  const int gjn = min(gjc, gw - gj0);
  const int Kp = n * ph * pw;                 // elements per patch position
  const int xv = gjn * pw / LV;
  const uint8_t* src = img + ((size_t)b * Ctot * H + (size_t)gi * ph) * W + (size_t)gj0 * pw;
  for (int e = threadIdx.x; e < n * ph * xv; e += blockDim.x) {
    const int row = e / xv, x = (e - row * xv) * LV;     // row = k * ph + pi
    const int k = row / ph, pi = row - k * ph;
    float v[LV];
    lookup_row<LV>(src + ((size_t)sel_channel_u8(sel, k, Ctot) * H + pi) * W + x, tab + k * 256, v);
    place_row<TO, LV, 4>(tile, Kp, pw, row, x, v);
  }
  __syncthreads();
  if constexpr (!COLWISE) {
    drain_bytes(out + (((size_t)b * gh + gi) * gw + gj0) * Kp, tile, gjn * Kp * (int)sizeof(TO), 16);
  } else {
    constexpr int EV = 16 / sizeof(TO);
    const int pv = Kp / EV;                   // 16-byte vectors per patch position (pw % 8 == 0)
    for (int e = threadIdx.x; e < gjn * pv; e += blockDim.x) {
      const int gj = e / pv, r = e - gj * pv;
      TO* dst = out + (((size_t)b * gw + gj0 + gj) * gh + gi) * Kp;
      reinterpret_cast<u32x4*>(dst)[r] = reinterpret_cast<const u32x4*>(tile)[e];
    }
  }
}

// ---- Mixup / CutMix over the two images of a pair -------------------------------------------------------------------
// The looked-up values are fp32, so the pixels are mixed as glue.hip's mix_pixels<float> mixes an fp32 image: each
// product an fp32 value of its own (the opaque copy keeps -ffast-math from contracting it into the sum), then the sum.
__device__ __forceinline__ float round_f32(float v) {
  asm("" : "+v"(v));
  return v;
}

enum { U8_MIX_COPY = 0, U8_MIX_MIXUP = 1, U8_MIX_CUTMIX = 2 };

template <int N>
__device__ __forceinline__ void mix_pixels_f32(const fv_mix_params& P, int mode, int y, int x0, const float (&a)[N], const float (&p)[N],
                                               float (&oa)[N], float (&op)[N]) {
#pragma clang fp reassociate(off) contract(off)
  if (mode == U8_MIX_MIXUP) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
      oa[k] = round_f32(round_f32(a[k] * P.lam) + round_f32(p[k] * P.one_minus_lam));
      op[k] = round_f32(round_f32(p[k] * P.lam) + round_f32(a[k] * P.one_minus_lam));
    }
  } else {
    // (plain & on the flags, no short-circuit: with `&&` the compiler turned the row test into a branch around the selects
    // and, in the 2-pixel form, left element 0 of rows outside the box unwritten -- tests/test_erasing_gpu.py, the LV 2 case)
    const bool in_rows = (mode == U8_MIX_CUTMIX) & (y >= P.yl) & (y < P.yh);
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const bool in_box = in_rows & (x0 + k >= P.xl) & (x0 + k < P.xh);
      oa[k] = in_box ? p[k] : a[k];
      op[k] = in_box ? a[k] : p[k];
    }
  }
}

template <typename TO, int LV, int PV, bool ERASE>
__global__ __launch_bounds__(U8_MIX_THREADS) void patch_unfold_mix_u8_kernel(const uint8_t* __restrict__ img, const float* __restrict__ table,
                                                                            TO* __restrict__ out, const fv_mix_params* __restrict__ mp,
                                                                            int B, int C, int H, int W, int ph, int pw, int gw, int sw,
                                                                            int tile_bytes, const int32_t* __restrict__ erase) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const fv_mix_params P = *mp;
  const int mode = P.use_cutmix ? U8_MIX_CUTMIX : (P.lam == 1.f ? U8_MIX_COPY : U8_MIX_MIXUP);
  TO* tile_a = reinterpret_cast<TO*>(smem);
  TO* tile_p = reinterpret_cast<TO*>(smem + tile_bytes);
  float* tab = reinterpret_cast<float*>(smem + 2 * tile_bytes);
  stage_table(tab, table, C);
  __syncthreads();
  const int gj0 = blockIdx.x * U8_MIX_GJ, gi = blockIdx.y, ba = blockIdx.z, bp = B - 1 - ba;
  const int gjn = min(U8_MIX_GJ, gw - gj0);
  const int Kp = C * ph * pw;                 // elements per patch row
  const int xv = gjn * pw / LV;
  const size_t org = (size_t)gi * ph * W + (size_t)gj0 * pw;
  const uint8_t* src_a = img + (size_t)ba * C * H * W + org;
  const uint8_t* src_p = img + (size_t)bp * C * H * W + org;
  fv_erase::Key ek = {};
  fv_erase::Box eba = {}, ebp = {};
  if constexpr (ERASE) {      // each image of the pair is erased with its own box, then the two are mixed
    ek = fv_erase::load_key(erase);
    eba = fv_erase::load_box(erase, ba);
    ebp = fv_erase::load_box(erase, bp);
  }
  for (int e = threadIdx.x; e < C * ph * xv; e += blockDim.x) {
    const int row = e / xv, x = (e - row * xv) * LV;     // row = c * ph + pi
    const int c = row / ph, pi = row - c * ph;
    const size_t off = ((size_t)c * H + pi) * W + x;
    float a[LV], p[LV], ra[LV], rp[LV];
    lookup_row<LV>(src_a + off, tab + c * 256, a);
    lookup_row<LV>(src_p + off, tab + c * 256, p);
    if constexpr (ERASE) {
      fv_erase::erase_segment<LV>(ek, eba, ba, c, gi * ph + pi, gj0 * pw + x, a);
      fv_erase::erase_segment<LV>(ek, ebp, bp, c, gi * ph + pi, gj0 * pw + x, p);
    }
    mix_pixels_f32<LV>(P, mode, gi * ph + pi, gj0 * pw + x, a, p, ra, rp);
    place_row<TO, LV, PV>(tile_a, Kp, pw, row, x, ra);
    place_row<TO, LV, PV>(tile_p, Kp, pw, row, x, rp);
  }
  __syncthreads();
  const size_t chunk = ((size_t)gi * gw + gj0) * Kp, image = (size_t)gridDim.y * gw * Kp;
  drain_bytes(out + (size_t)ba * image + chunk, tile_a, gjn * Kp * (int)sizeof(TO), sw);
  drain_bytes(out + (size_t)bp * image + chunk, tile_p, gjn * Kp * (int)sizeof(TO), sw);
}

// ---- host side ------------------------------------------------------------------------------------------------------
// Bytes per image load: every segment a thread loads starts at base + (a multiple of W) + (a multiple of gjc * pw) + (a
// multiple of LV) and the segments of a chunk are gjc * pw or W - k * gjc * pw bytes long, so LV may be any power of two
// that divides W, gjc * pw and the base address.
int load_bytes(const void* img, int W, int chunk_px) {
  for (int lv = 16; lv > 1; lv >>= 1)
    if (W % lv == 0 && chunk_px % lv == 0 && ((uintptr_t)img % lv) == 0) return lv;
  return 1;
}

// Bytes per tile store (glue.hip's unfold_store_bytes): every chunk starts and ends on a multiple of gcd(gw, gjc) patches.
int store_bytes(int gw, int gjc, size_t patch_bytes) {
  int a = gw, b = gjc;
  while (b) { const int t = a % b; a = b; b = t; }
  const size_t unit = (size_t)a * patch_bytes;
  return unit % 16 == 0 ? 16 : unit % 8 == 0 ? 8 : 4;
}

bool out_dt_ok(int dt) { return dt == FV_F32 || dt == FV_BF16; }

}  // namespace

// one of the (LV, PV) forms of a plain / pair kernel: PV = 4 where the patch width is a multiple of 4, else pairs
#define FV_U8_FORMS(LAUNCH, TO, RE)                               \
  do {                                                            \
    if (lv == 16) { if (pv4) LAUNCH(TO, 16, 4, RE); else LAUNCH(TO, 16, 2, RE); } \
    else if (lv == 8) { if (pv4) LAUNCH(TO, 8, 4, RE); else LAUNCH(TO, 8, 2, RE); } \
    else if (lv == 4) { if (pv4) LAUNCH(TO, 4, 4, RE); else LAUNCH(TO, 4, 2, RE); } \
    else LAUNCH(TO, 2, 2, RE);                                    \
  } while (0)
// the plain / the _re entry point: the same launch with ERASE false / true
#define FV_U8_DTYPES(LAUNCH)                                      \
  do {                                                            \
    if (erase) { if (out_dtype == FV_BF16) FV_U8_FORMS(LAUNCH, bf16_t, true); else FV_U8_FORMS(LAUNCH, float, true); } \
    else { if (out_dtype == FV_BF16) FV_U8_FORMS(LAUNCH, bf16_t, false); else FV_U8_FORMS(LAUNCH, float, false); } \
  } while (0)

// erase == nullptr: the plain launch; else the block of the _re entry point
static int unfold_u8_launch(const uint8_t* img, const float* table, void* out, int out_dtype, int batch, int chans, int height,
                            int width, int ph, int pw, const int32_t* erase, fv_stream_t stream) {
  FV_CHECK(img && table && out, "patch_unfold_u8: null pointer");
  FV_CHECK(out_dt_ok(out_dtype), "patch_unfold_u8: the output must be fp32 or bf16");
  FV_CHECK(batch > 0 && chans > 0 && ph > 0 && pw > 0 && height >= ph && width >= pw, "patch_unfold_u8: empty dimension");
  FV_CHECK(height % ph == 0 && width % pw == 0, "patch_unfold_u8: image %dx%d is not whole %dx%d patches", height, width, ph, pw);
  FV_CHECK(pw % 2 == 0 && pw >= 8 && ((uintptr_t)img & 1) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)table & 15) == 0,
           "patch_unfold_u8: patch width must be even and at least 8, the image 2-byte and the table and the output 16-byte aligned");
  const int gh = height / ph, gw = width / pw;
  const size_t osz = out_dtype == FV_F32 ? 4 : 2;
  const size_t tile = (size_t)U8_GJ * chans * ph * pw * osz;
  const size_t smem = tile + (size_t)chans * 1024;
  FV_CHECK(smem <= 64 * 1024, "patch_unfold_u8: %d x %d x %d patches and the table do not fit the workgroup's LDS", chans, ph, pw);
  FV_CHECK(gh <= 65535 && batch <= 65535, "patch_unfold_u8: grid too large");
  const dim3 grid(fv_cdiv(gw, U8_GJ), gh, batch), block(256);
  hipStream_t st = (hipStream_t)stream;
  const int lv = load_bytes(img, width, U8_GJ * pw);
  const bool pv4 = pw % 4 == 0;
  const int sw = store_bytes(gw, U8_GJ, (size_t)chans * ph * pw * osz);
#define FV_U8_PLAIN(TO, LV, PV, RE) hipLaunchKernelGGL((patch_unfold_u8_kernel<TO, LV, PV, RE>), grid, block, smem, st, img, table, (TO*)out, chans, height, width, ph, pw, gw, sw, (int)tile, erase)
  FV_U8_DTYPES(FV_U8_PLAIN);
#undef FV_U8_PLAIN
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_patch_unfold_u8(const uint8_t* img, const float* table, void* out, int out_dtype, int batch, int chans,
                                  int height, int width, int ph, int pw, fv_stream_t stream) {
  return unfold_u8_launch(img, table, out, out_dtype, batch, chans, height, width, ph, pw, nullptr, stream);
}

extern "C" int fv_patch_unfold_u8_re(const uint8_t* img, const float* table, void* out, int out_dtype, int batch, int chans,
                                     int height, int width, int ph, int pw, const void* erase, fv_stream_t stream) {
  FV_CHECK(erase && ((uintptr_t)erase & 15) == 0, "patch_unfold_u8_re: the erase block must be a 16-byte aligned device pointer");
  return unfold_u8_launch(img, table, out, out_dtype, batch, chans, height, width, ph, pw, (const int32_t*)erase, stream);
}

static int unfold_mix_u8_launch(const uint8_t* img, const float* table, void* out, int out_dtype, int batch, int chans, int height,
                                int width, int ph, int pw, const void* mix, const int32_t* erase, fv_stream_t stream) {
  FV_CHECK(img && table && out && mix, "patch_unfold_mix_u8: null pointer");
  FV_CHECK(out_dt_ok(out_dtype), "patch_unfold_mix_u8: the output must be fp32 or bf16");
  FV_CHECK(batch > 0 && chans > 0 && ph > 0 && pw > 0 && height >= ph && width >= pw, "patch_unfold_mix_u8: empty dimension");
  FV_CHECK(batch % 2 == 0, "patch_unfold_mix_u8: batch mode pairs image b with image batch-1-b, the batch (%d) must be even", batch);
  FV_CHECK(height % ph == 0 && width % pw == 0, "patch_unfold_mix_u8: image %dx%d is not whole %dx%d patches", height, width, ph, pw);
  FV_CHECK(pw % 2 == 0 && pw >= 8 && ((uintptr_t)img & 1) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)table & 15) == 0,
           "patch_unfold_mix_u8: patch width must be even and at least 8, the image 2-byte and the table and the output 16-byte aligned");
  FV_CHECK(((size_t)chans * height * width) % 2 == 0, "patch_unfold_mix_u8: odd image size");
  const int gh = height / ph, gw = width / pw;
  const size_t osz = out_dtype == FV_F32 ? 4 : 2;
  const size_t tile = (size_t)U8_MIX_GJ * chans * ph * pw * osz;
  const size_t smem = 2 * tile + (size_t)chans * 1024;
  FV_CHECK(smem <= 64 * 1024, "patch_unfold_mix_u8: %d x %d x %d patches and the table do not fit the workgroup's LDS", chans, ph, pw);
  FV_CHECK(gh <= 65535 && batch / 2 <= 65535, "patch_unfold_mix_u8: grid too large");
  const dim3 grid(fv_cdiv(gw, U8_MIX_GJ), gh, batch / 2), block(U8_MIX_THREADS);
  hipStream_t st = (hipStream_t)stream;
  const fv_mix_params* mp = (const fv_mix_params*)mix;
  const int lv = load_bytes(img, width, U8_MIX_GJ * pw);
  const bool pv4 = pw % 4 == 0;
  const int sw = store_bytes(gw, U8_MIX_GJ, (size_t)chans * ph * pw * osz);
#define FV_U8_MIX(TO, LV, PV, RE) hipLaunchKernelGGL((patch_unfold_mix_u8_kernel<TO, LV, PV, RE>), grid, block, smem, st, img, table, (TO*)out, mp, batch, chans, height, width, ph, pw, gw, sw, (int)tile, erase)
  FV_U8_DTYPES(FV_U8_MIX);
#undef FV_U8_MIX
  FV_LAUNCH_CHECK();
  return FV_OK;
}

extern "C" int fv_patch_unfold_mix_u8(const uint8_t* img, const float* table, void* out, int out_dtype, int batch, int chans,
                                      int height, int width, int ph, int pw, const void* mix, fv_stream_t stream) {
  return unfold_mix_u8_launch(img, table, out, out_dtype, batch, chans, height, width, ph, pw, mix, nullptr, stream);
}

extern "C" int fv_patch_unfold_mix_u8_re(const uint8_t* img, const float* table, void* out, int out_dtype, int batch, int chans,
                                         int height, int width, int ph, int pw, const void* mix, const void* erase,
                                         fv_stream_t stream) {
  FV_CHECK(erase && ((uintptr_t)erase & 15) == 0, "patch_unfold_mix_u8_re: the erase block must be a 16-byte aligned device pointer");
  return unfold_mix_u8_launch(img, table, out, out_dtype, batch, chans, height, width, ph, pw, mix, (const int32_t*)erase, stream);
}

extern "C" int fv_patch_unfold_chan_u8(const uint8_t* img, const float* table, void* out, int out_dtype, int batch, int chans_total,
                                       int height, int width, int ph, int pw, const int32_t* sel, int n_sel, int colwise,
                                       fv_stream_t stream) {
  FV_CHECK(img && table && out, "patch_unfold_chan_u8: null pointer");
  FV_CHECK(out_dt_ok(out_dtype), "patch_unfold_chan_u8: the output must be fp32 or bf16");
  FV_CHECK(batch > 0 && chans_total > 0 && ph > 0 && pw > 0 && height >= ph && width >= pw, "patch_unfold_chan_u8: empty dimension");
  FV_CHECK(n_sel > 0 && n_sel <= chans_total, "patch_unfold_chan_u8: %d selected channels of %d", n_sel, chans_total);
  FV_CHECK(height % ph == 0 && width % pw == 0, "patch_unfold_chan_u8: image %dx%d is not whole %dx%d patches", height, width, ph, pw);
  FV_CHECK(pw % 8 == 0 && ((uintptr_t)img & 3) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)table & 15) == 0,
           "patch_unfold_chan_u8: patch width must be a multiple of 8, the image 4-byte and the table and the output 16-byte aligned");
  const int gh = height / ph, gw = width / pw;
  const size_t osz = out_dtype == FV_F32 ? 4 : 2;
  // patches per workgroup as fv_patch_unfold_chan cuts them: at most 16, a tile of at most 32 KB, the patch row in equal chunks
  const size_t per_patch = (size_t)n_sel * ph * pw * osz;
  const size_t tab_bytes = (size_t)n_sel * 1024;
  FV_CHECK(per_patch + tab_bytes <= 64 * 1024, "patch_unfold_chan_u8: %d x %d x %d patches and the table do not fit the workgroup's LDS", n_sel, ph, pw);
  int fit = (int)((32 * 1024) / per_patch);
  fit = fit < 1 ? 1 : (fit > U8_GJ ? U8_GJ : fit);
  const int gjc = fv_cdiv(gw, fv_cdiv(gw, fit));
  const size_t tile = gjc * per_patch;
  const size_t smem = tile + tab_bytes;
  FV_CHECK(gh <= 65535 && batch <= 65535, "patch_unfold_chan_u8: grid too large");
  const dim3 grid(fv_cdiv(gw, gjc), gh, batch), block(256);
  hipStream_t st = (hipStream_t)stream;
  const int lv = load_bytes(img, width, gjc * pw);      // 16, 8 or 4: pw % 8 == 0 and the base is 4-byte aligned
#define FV_U8_CHAN2(TO, LV, CW) hipLaunchKernelGGL((patch_unfold_chan_u8_kernel<TO, LV, CW>), grid, block, smem, st, img, table, (TO*)out, sel, n_sel, chans_total, height, width, ph, pw, gw, gjc, (int)tile)
#define FV_U8_CHAN(TO, LV) do { if (colwise) FV_U8_CHAN2(TO, LV, true); else FV_U8_CHAN2(TO, LV, false); } while (0)
#define FV_U8_CHAN_LV(TO) do { if (lv == 16) FV_U8_CHAN(TO, 16); else if (lv == 8) FV_U8_CHAN(TO, 8); else FV_U8_CHAN(TO, 4); } while (0)
  if (out_dtype == FV_BF16) FV_U8_CHAN_LV(bf16_t);
  else FV_U8_CHAN_LV(float);
#undef FV_U8_CHAN_LV
#undef FV_U8_CHAN
#undef FV_U8_CHAN2
  FV_LAUNCH_CHECK();
  return FV_OK;
}
#undef FV_U8_DTYPES
#undef FV_U8_FORMS
