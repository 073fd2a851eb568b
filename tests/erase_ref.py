"""Reference of random erasing for the tests, numpy / pure Python only: an independent restatement of timm's box loop, of
Philox4x32-10 and of the Box-Muller mapping (in fp64) that include/fastvim_hip.h specifies for the erase block's noise."""
import math

import numpy as np

M32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------- boxes
def draw_boxes(rng, batch, H, W, probability, min_area=0.02, max_area=1 / 3, min_aspect=0.3, max_aspect=None):
    """timm.data.random_erasing.RandomErasing._erase with count 1, for samples 0 .. batch-1, consuming ``rng`` (the
    ``random`` module or a ``random.Random``) as it does.  ``(top, left, h, w)`` per sample, ``(0, 0, 0, 0)``: not erased."""
    lo, hi = math.log(min_aspect), math.log(max_aspect or 1 / min_aspect)
    out = []
    for _ in range(batch):
        box = (0, 0, 0, 0)
        if rng.random() > probability:
            out.append(box)
            continue
        area = H * W
        for _attempt in range(10):
            target = rng.uniform(min_area, max_area) * area / 1
            ar = math.exp(rng.uniform(lo, hi))
            h = int(round(math.sqrt(target * ar)))
            w = int(round(math.sqrt(target / ar)))
            if w < W and h < H:
                top = rng.randint(0, H - h)
                left = rng.randint(0, W - w)
                if h > 0 and w > 0:
                    box = (top, left, h, w)
                break
        out.append(box)
    return out


# ---------------------------------------------------------------------------------------------- Philox4x32-10
def philox4x32_10(counter, key):
    """Scalar form: ``counter`` 4 words, ``key`` 2 words -> 4 words (Salmon et al., SC'11)."""
    c0, c1, c2, c3 = (int(v) & M32 for v in counter)
    k0, k1 = (int(v) & M32 for v in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def philox4x32_10_np(c0, c1, c2, c3, key):
    """The same over uint64 arrays that hold 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) & np.uint64(M32) for v in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(key[0]) & M32, int(key[1]) & M32
    m = np.uint64(M32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)) & m, p1 & m, ((p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)) & m, p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


# ---------------------------------------------------------------------------------------------- noise
def box_muller(ra, rb):
    """Two 32-bit words -> two standard-normal values, fp64: u1 = ((ra >> 8) + 1) 2^-24, u2 = (rb >> 8) 2^-24."""
    u1 = ((np.asarray(ra, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (np.asarray(rb, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    rad = np.sqrt(-2.0 * np.log(u1))
    return rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2)


def noise_at(key, b, c, y, x):
    """The noise of pixel (b, c, y, x), fp64 (scalar form, from the scalar Philox)."""
    r = philox4x32_10((x >> 2, y, c, b), key)
    pair = (r[2], r[3]) if x & 2 else (r[0], r[1])
    z = box_muller(pair[0], pair[1])
    return float(z[x & 1])


def noise_box(key, b, C, top, left, h, w):
    """fp64 (C, h, w): the noise of sample b inside its box."""
    c = np.arange(C).reshape(C, 1, 1)
    y = (top + np.arange(h)).reshape(1, h, 1)
    x = (left + np.arange(w)).reshape(1, 1, w)
    c, y, x = np.broadcast_arrays(c, y, x)
    r = philox4x32_10_np(x >> 2, y, c, np.full_like(x, b), key)
    hi = (x & 2) != 0
    za, zb = box_muller(np.where(hi, r[2], r[0]), np.where(hi, r[3], r[1]))
    return np.where((x & 1) != 0, zb, za)
