// Random erasing of a float NCHW batch (fv_random_erase): the eager form of what the ERASE forms of the uint8 patch
// unfolds (unfold_u8.hip) do on their way into the tile.  Boxes, mode and noise key are read from the erase block in
// device memory when the kernel runs (include/fastvim_hip.h); the noise is erase_noise.h's, so all three launches write
// the same bits for the same key.
//
// A thread owns EV consecutive pixels of an image row -- 16 bytes where the width and the two addresses allow, else 8, 4
// or one element, as the unfold kernels fall back -- and copies them as raw words; only a segment that meets its sample's
// box is unpacked, erased and packed again (the fp32 noise rounded once to the storage type).  In place (out == x)
// nothing outside a box is read or written.
#include "common.h"
#include "erase_noise.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// EV elements of T as raw storage: NW dwords (or one 16-bit word for a single bf16)
template <typename T, int EV> struct Raw {
  static constexpr int NB = EV * (int)sizeof(T);
  static constexpr int NW = NB >= 4 ? NB / 4 : 1;
  uint32_t w[NW];

  __device__ __forceinline__ void ld(const T* p) {
    if constexpr (NB == 16) {
      const u32x4 t = *reinterpret_cast<const u32x4*>(p);
      w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
    } else if constexpr (NB == 8) {
      const u32x2 t = *reinterpret_cast<const u32x2*>(p);
      w[0] = t.x; w[1] = t.y;
    } else if constexpr (NB == 4) {
      w[0] = *reinterpret_cast<const uint32_t*>(p);
    } else {
      w[0] = *reinterpret_cast<const uint16_t*>(p);
    }
  }
  __device__ __forceinline__ void st(T* p) const {
    if constexpr (NB == 16) {
      u32x4 t; t.x = w[0]; t.y = w[1]; t.z = w[2]; t.w = w[3];
      *reinterpret_cast<u32x4*>(p) = t;
    } else if constexpr (NB == 8) {
      u32x2 t; t.x = w[0]; t.y = w[1];
      *reinterpret_cast<u32x2*>(p) = t;
    } else if constexpr (NB == 4) {
      *reinterpret_cast<uint32_t*>(p) = w[0];
    } else {
      *reinterpret_cast<uint16_t*>(p) = (uint16_t)w[0];
    }
  }
  __device__ __forceinline__ void unpack(float (&v)[EV]) const {
#pragma unroll
    for (int j = 0; j < EV; ++j) {
      if constexpr (sizeof(T) == 4) v[j] = __uint_as_float(w[j]);
      else v[j] = bf16_bits_to_f32((uint16_t)(w[j >> 1] >> (16 * (j & 1))));
    }
  }
  __device__ __forceinline__ void pack(const float (&v)[EV]) {
    if constexpr (sizeof(T) == 4) {
#pragma unroll
      for (int j = 0; j < EV; ++j) w[j] = __float_as_uint(v[j]);
    } else if constexpr (EV == 1) {
      w[0] = f32_to_bf16_bits(v[0]);
    } else {
#pragma unroll
      for (int j = 0; j < EV; j += 2) w[j >> 1] = pack_bf16x2(v[j], v[j + 1]);
    }
  }
};

// grid (chunks of an image, batch): x and out may be the same buffer, so neither is __restrict__
template <typename T, int EV>
__global__ __launch_bounds__(256) void random_erase_kernel(const T* x, T* out, const int32_t* __restrict__ erase, int n, int H, int W) {
  const int b = blockIdx.y;
  const fv_erase::Key ek = fv_erase::load_key(erase);
  const fv_erase::Box eb = fv_erase::load_box(erase, b);
  const bool inplace = x == out;
  if (inplace && eb.h <= 0) return;
  const size_t base = (size_t)b * n;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n / EV; e += gridDim.x * blockDim.x) {
    const int i = e * EV, row = i / W, x0 = i - row * W;      // row = c * H + y; W % EV == 0 keeps the segment in it
    const int c = row / H, y = row - c * H;
    const bool hit = fv_erase::hits(eb, y, x0, EV);
    if (inplace && !hit) continue;
    Raw<T, EV> r;
    r.ld(x + base + i);
    if (hit) {
      float v[EV];
      r.unpack(v);
      fv_erase::erase_segment<EV>(ek, eb, b, c, y, x0, v);
      r.pack(v);
    }
    r.st(out + base + i);
  }
}

}  // namespace

extern "C" int fv_random_erase(const void* x, void* out, int dtype, int batch, int chans, int height, int width, const void* erase,
                               fv_stream_t stream) {
  FV_CHECK(x && out && erase, "random_erase: null pointer");
  FV_CHECK(dtype == FV_F32 || dtype == FV_BF16, "random_erase: dtype must be fp32 or bf16");
  FV_CHECK(batch > 0 && chans > 0 && height > 0 && width > 0, "random_erase: empty dimension");
  FV_CHECK(((uintptr_t)erase & 15) == 0, "random_erase: the erase block must be 16-byte aligned");
  const long n = (long)chans * height * width;
  FV_CHECK(n < (1l << 31) && batch <= 65535, "random_erase: image or batch too large");
  const size_t esz = dtype == FV_F32 ? 4 : 2;
  FV_CHECK(((uintptr_t)x % esz) == 0 && ((uintptr_t)out % esz) == 0, "random_erase: misaligned tensor");
  if (x != out) {
    const uintptr_t xa = (uintptr_t)x, oa = (uintptr_t)out, bytes = (uintptr_t)batch * n * esz;
    FV_CHECK(xa + bytes <= oa || oa + bytes <= xa, "random_erase: x and out overlap (only out == x is allowed)");
  }
  // elements per thread: the largest of 16, 8, 4 bytes (fp32: 4, 2, 1 elements; bf16: 8, 4, 2) that divides the row and
  // both addresses -- every image starts a multiple of the row from the base -- else one element
  int ev = 1;
  for (int nb = 16; nb >= 4; nb >>= 1) {
    const int k = nb / (int)esz;
    if (width % k == 0 && ((uintptr_t)x % nb) == 0 && ((uintptr_t)out % nb) == 0) { ev = k; break; }
  }
  const long work = n / ev;
  const dim3 grid(fv_cdiv(work, 256) < 1024 ? fv_cdiv(work, 256) : 1024, batch), block(256);
  hipStream_t st = (hipStream_t)stream;
  const int32_t* blk = (const int32_t*)erase;
#define FV_RE(T, EV) hipLaunchKernelGGL((random_erase_kernel<T, EV>), grid, block, 0, st, (const T*)x, (T*)out, blk, (int)n, height, width)
  if (dtype == FV_F32) {
    if (ev == 4) FV_RE(float, 4); else if (ev == 2) FV_RE(float, 2); else FV_RE(float, 1);
  } else {
    if (ev == 8) FV_RE(bf16_t, 8); else if (ev == 4) FV_RE(bf16_t, 4); else if (ev == 2) FV_RE(bf16_t, 2); else FV_RE(bf16_t, 1);
  }
#undef FV_RE
  FV_LAUNCH_CHECK();
  return FV_OK;
}
