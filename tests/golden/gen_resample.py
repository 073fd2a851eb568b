"""Writes tests/golden/resample.npz: a dozen small inputs and what PIL itself computes from them --
``Image.fromarray(a).crop(box).resize((o_w, o_h), Image.BICUBIC)`` -- so that machines without PIL can hold the numpy
reference (tests/resample_ref.py) and the kernels to PIL's bytes.  Run once with PIL installed: ``python
tests/golden/gen_resample.py``; the arrays are ``in_K`` (H, W, 3) uint8, ``meta_K`` = (top, left, h, w, o_h, o_w) and
``out_K`` (o_h, o_w, 3) uint8.  Every output side is in [8, 32], the window range of the device tests."""
import os

import numpy as np
from PIL import Image

# (H, W, crop or None, o_h, o_w, binary)
CASES = [
    (16, 16, None, 16, 16, False),            # identity
    (5, 7, None, 16, 16, False),              # upscale
    (33, 29, None, 16, 16, True),             # 0 / 255 only: reaches the clip on both sides
    (1, 1, None, 8, 8, False),                # one pixel
    (9, 50, None, 16, 24, False),
    (40, 61, None, 18, 27, False),            # the validation resize: short side to 18, long side int(18 * 61 / 40)
    (128, 16, None, 8, 8, True),              # scale exactly 16 down, 2 across
    (30, 40, (3, 5, 20, 22), 12, 10, False),  # taps clamp at the crop's edge, not the image's
    (17, 90, None, 8, 9, False),              # scale 10 across
    (24, 24, None, 24, 24, True),
    (8, 8, None, 24, 16, False),
    (50, 31, (0, 0, 50, 31), 13, 8, False),
]


def main():
    rng = np.random.default_rng(20240)
    out = {}
    for k, (H, W, crop, o_h, o_w, binary) in enumerate(CASES):
        a = (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8) if binary else rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        top, left, h, w = crop or (0, 0, H, W)
        img = Image.fromarray(a).crop((left, top, left + w, top + h)).resize((o_w, o_h), Image.BICUBIC)
        out[f"in_{k}"] = a
        out[f"meta_{k}"] = np.array([top, left, h, w, o_h, o_w], np.int32)
        out[f"out_{k}"] = np.asarray(img)
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "resample.npz"), **out)


if __name__ == "__main__":
    main()
