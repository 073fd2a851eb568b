"""numpy restatement of the MAE masking noise (include/fastvim_hip.h, at ``fv_mae_noise``; csrc/mask_noise.h) on the
independent Philox4x32-10 of tests/erase_ref.py, and the plan of that noise through tests/mae_tokens_ref.plan_ref.

The noise of sample b, token l under ``(seed, counter)`` is ``float(w >> 8) * 2**-24`` with ``w`` word ``l & 3`` of
Philox4x32-10(key = (seed & 0xffffffff, seed >> 32), counter = (l >> 2, b, counter & 0xffffffff, counter >> 32))."""
import numpy as np
import torch

import erase_ref
import mae_tokens_ref

M32 = 0xFFFFFFFF


def key_words(seed, counter):
    """(k0, k1, step_lo, step_hi)"""
    return seed & M32, (seed >> 32) & M32, counter & M32, (counter >> 32) & M32


def noise_words(seed, counter, B, L):
    """(B, L) uint64 array of the 32-bit words ``w``."""
    k0, k1, s0, s1 = key_words(seed, counter)
    b = np.arange(B, dtype=np.uint64).reshape(B, 1)
    l = np.arange(L, dtype=np.uint64).reshape(1, L)
    b, l = np.broadcast_arrays(b, l)
    r = erase_ref.philox4x32_10_np(l >> np.uint64(2), b, np.full_like(l, s0), np.full_like(l, s1), (k0, k1))
    lane = l & np.uint64(3)
    return np.select([lane == 0, lane == 1, lane == 2], [r[0], r[1], r[2]], r[3])


def noise_f64(seed, counter, B, L):
    """The noise in fp64: every value is k 2^-24 with an integer k < 2^24, so the fp32 cast is exact."""
    return (noise_words(seed, counter, B, L) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def noise(seed, counter, B, L):
    """(B, L) fp32 CPU tensor."""
    return torch.from_numpy(noise_f64(seed, counter, B, L).astype(np.float32))


def noise_at(seed, counter, b, l):
    """One value from the SCALAR Philox (fp64)."""
    k0, k1, s0, s1 = key_words(seed, counter)
    w = erase_ref.philox4x32_10((l >> 2, b, s0, s1), (k0, k1))[l & 3]
    return (w >> 8) * 2.0 ** -24


def plan(seed, counter, B, H, W, K):
    """``mae_tokens_ref.plan_ref`` of the noise: the twelve tensors of a ``TokenPlan``."""
    return mae_tokens_ref.plan_ref(noise(seed, counter, B, H * W), H, W, K)


# the case that exercises the stable order: sample 5 of this tensor holds repeated values
TIE_CASE = {"seed": 2, "counter": 1, "B": 8, "L": 1024, "sample": 5}
