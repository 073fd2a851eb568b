// Random erasing: the erase block (include/fastvim_hip.h, at fv_random_erase) and the ONE definition of the noise that
// every kernel writes inside a box -- fv_random_erase (erase.hip) and the ERASE forms of the uint8 patch unfolds
// (unfold_u8.hip).
//
// The value at (b, c, y, x) is a function of (key0, key1, b, c, y, x) and of nothing else: Philox4x32-10 with key
// (key0, key1) and counter (x >> 2, y, c, b); its four output words serve the four pixels x & ~3 .. x | 3: words 0, 1 go
// through Box-Muller (cos, sin) to pixels 0, 1, words 2, 3 to pixels 2, 3.  A caller that holds 4 or more consecutive
// pixels works group by group; one that holds 2 (or 1) computes the group's words and the one Box-Muller pair it needs.
//
// The library is built with -ffast-math, and the function is inlined into kernels of different shapes that must agree bit
// for bit.  So every step is ONE instruction whose operands are pinned by opaque copies: the integer-to-float
// conversions and the power-of-two scale are exact, log2 / sqrt / sin / cos are the hardware instructions (v_log_f32,
// v_sqrt_f32, v_sin_f32, v_cos_f32 -- the last two take their argument in revolutions, which is what u2 is) named by
// builtin, not libm calls that the flags could expand one way here and another way there, and the two products are
// fenced so that no caller can contract them into its own arithmetic.
#pragma once
#include "common.h"

namespace fv_erase {

struct Key {
  uint32_t k0, k1;
  int mode;      // FV_ERASE_CONST / FV_ERASE_PIXEL
};
struct Box {
  int top, left, h, w;      // h <= 0: no erase
};

// the header of the block and sample b's record (b, and so every load, is uniform over a workgroup in all callers)
__device__ __forceinline__ Key load_key(const int32_t* __restrict__ blk) {
  Key k;
  k.k0 = (uint32_t)blk[0];
  k.k1 = (uint32_t)blk[1];
  k.mode = blk[2];
  return k;
}
__device__ __forceinline__ Box load_box(const int32_t* __restrict__ blk, int b) {
  Box e = {0, 0, 0, 0};
  if (b < blk[3]) {
    const int32_t* r = blk + 4 + 4 * b;
    e.top = r[0]; e.left = r[1]; e.h = r[2]; e.w = r[3];
  }
  return e;
}

// do pixels x0 .. x0 + n - 1 of row y meet the box?
__device__ __forceinline__ bool hits(const Box& e, int y, int x0, int n) {
  return e.h > 0 && y >= e.top && y < e.top + e.h && x0 < e.left + e.w && x0 + n > e.left;
}

__device__ __forceinline__ float opaque(float v) {
  asm("" : "+v"(v));
  return v;
}

__device__ __forceinline__ void philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t (&r)[4]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// two words -> two standard-normal values: sqrt(-2 ln u1) * (cos, sin)(2 pi u2)
__device__ __forceinline__ void box_muller(uint32_t ra, uint32_t rb, float& z0, float& z1) {
  const float u1 = opaque((float)((ra >> 8) + 1u) * 0x1p-24f);      // (0, 1], exact
  const float u2 = opaque((float)(rb >> 8) * 0x1p-24f);             // [0, 1), exact
  const float t = opaque(__builtin_amdgcn_logf(u1) * -1.3862943611198906f);      // log2(u1) * (-2 ln 2) >= 0
  const float rad = opaque(__builtin_amdgcn_sqrtf(t));
  const float cs = opaque(__builtin_amdgcn_cosf(u2)), sn = opaque(__builtin_amdgcn_sinf(u2));
  z0 = opaque(rad * cs);
  z1 = opaque(rad * sn);
}

// the four values of pixel group xg = x >> 2 of row y, channel c, sample b
__device__ __forceinline__ void noise4(const Key& K, int b, int c, int y, int xg, float (&z)[4]) {
  uint32_t r[4];
  philox4x32_10(K.k0, K.k1, (uint32_t)xg, (uint32_t)y, (uint32_t)c, (uint32_t)b, r);
  box_muller(r[0], r[1], z[0], z[1]);
  box_muller(r[2], r[3], z[2], z[3]);
}

// v = pixels x0 .. x0 + N - 1 of row y, channel c, sample b (x0 a multiple of min(N, 4), N 1, 2 or a multiple of 4): the
// ones inside the box are replaced.  Noise is made per group of four straight into v -- no second array -- and only by
// lanes whose group meets the box.
template <int N>
__device__ __forceinline__ void erase_segment(const Key& K, const Box& e, int b, int c, int y, int x0, float (&v)[N]) {
  static_assert(N == 1 || N == 2 || N % 4 == 0, "erase_segment: 1, 2 or whole groups of 4 pixels");
  const int xl = e.left, xh = e.left + e.w;
  if constexpr (N >= 4) {
#pragma unroll
    for (int g = 0; g < N; g += 4) {
      if (hits(e, y, x0 + g, 4)) {
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (K.mode == FV_ERASE_PIXEL) noise4(K, b, c, y, (x0 + g) >> 2, z);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int x = x0 + g + k;
          v[g + k] = (x >= xl && x < xh) ? z[k] : v[g + k];
        }
      }
    }
  } else {
    if (hits(e, y, x0, N)) {
      float z0 = 0.f, z1 = 0.f;
      if (K.mode == FV_ERASE_PIXEL) {
        uint32_t r[4];
        philox4x32_10(K.k0, K.k1, (uint32_t)(x0 >> 2), (uint32_t)y, (uint32_t)c, (uint32_t)b, r);
        const bool hi = (x0 & 2) != 0;
        box_muller(hi ? r[2] : r[0], hi ? r[3] : r[1], z0, z1);
      }
      if constexpr (N == 2) {
        v[0] = (x0 >= xl && x0 < xh) ? z0 : v[0];
        v[1] = (x0 + 1 >= xl && x0 + 1 < xh) ? z1 : v[1];
      } else {
        v[0] = (x0 & 1) ? z1 : z0;      // (hits: the one pixel is inside)
      }
    }
  }
}

}  // namespace fv_erase
