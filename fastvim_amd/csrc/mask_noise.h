// MAE masking noise from a key: the key block (include/fastvim_hip.h, at fv_mae_noise) and the ONE definition of the noise
// that fv_mae_noise writes and fv_mae_mask_plan_keyed ranks without ever storing it (mae_tokens.hip).
//
// The noise of sample b, token l is u = float(w >> 8) * 2^-24 with w = word (l & 3) of Philox4x32-10 under key (k0, k1) and
// counter (l >> 2, b, step_lo, step_hi): a function of the block's four words, b and l and of nothing else.  Both steps
// are exact -- a 24-bit integer converts to fp32 without rounding and the scale is a power of two whose results are all
// normal numbers or zero -- so -ffast-math has nothing to reorder and every caller gets the same bits.  u lies in [0, 1)
// on the 2^-24 grid, the resolution of torch.rand.  The rounds are the erase noise's (erase_noise.h), shared, not copied.
#pragma once
#include "erase_noise.h"

namespace fv_mask {

struct Key {
  uint32_t k0, k1, step_lo, step_hi;
};

// the block's four words (uniform over the launch)
__device__ __forceinline__ Key load_key(const int32_t* __restrict__ blk) {
  Key k;
  k.k0 = (uint32_t)blk[0];
  k.k1 = (uint32_t)blk[1];
  k.step_lo = (uint32_t)blk[2];
  k.step_hi = (uint32_t)blk[3];
  return k;
}

__device__ __forceinline__ float unit(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }

// the noise of tokens 4 g .. 4 g + 3 of sample b
__device__ __forceinline__ void noise4(const Key& K, int b, int g, float (&u)[4]) {
  uint32_t r[4];
  fv_erase::philox4x32_10(K.k0, K.k1, (uint32_t)g, (uint32_t)b, K.step_lo, K.step_hi, r);
#pragma unroll
  for (int k = 0; k < 4; ++k) u[k] = unit(r[k]);
}

}  // namespace fv_mask
