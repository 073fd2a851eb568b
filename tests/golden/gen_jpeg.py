"""Writes tests/golden/jpeg_cases.npz: JPEG files PIL encoded and the RGB PIL decodes them to
(``Image.open(...).convert("RGB")``), for tests/test_jpeg_cpu.py, tests/test_jpeg_gpu.py and tools/jpeg_host_check.cpp.
Run where PIL (with libjpeg-turbo) is: ``python tests/golden/gen_jpeg.py``.  Content is seeded; the file also records
PIL's and libjpeg-turbo's versions.

The list is the smallest that covers every branch: the six sizes (one block, non-multiples of every MCU, 1 x 1, more than
one MCU row and column), the four sampling classes, three qualities (20: long zero runs and ZRL; 100: table entries of 1,
long codes), optimised Huffman tables, a restart interval of one MCU and of one MCU row, smooth / noise / hard-edged
content (the last reaches the clamp), and one progressive file for the fallback."""
import io
import os

import numpy as np
import PIL
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = ((8, 8), (17, 23), (33, 47), (64, 80), (9, 130), (1, 1))
CLASSES = ("444", "422", "420", "gray")


def content(kind, H, W, seed):
    rng = np.random.default_rng(seed)
    if kind == "smooth":
        y, x = np.mgrid[0:H, 0:W]
        return np.stack([(y * 5 + x * 3) % 256, 255 - (x * 2) % 256, (y * 2 + x + 100) % 256], 2).astype(np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    a = (rng.integers(0, 2, ((H + 3) // 4, (W + 3) // 4, 3)) * 255).astype(np.uint8)      # 4 x 4 blocks of 0 / 255
    return np.kron(a, np.ones((4, 4, 1), np.uint8))[:H, :W]


def encode(a, cls, **kw):
    b = io.BytesIO()
    if cls == "gray":
        Image.fromarray(a).convert("L").save(b, "JPEG", **kw)
    else:
        Image.fromarray(a).save(b, "JPEG", subsampling=CLASSES.index(cls), **kw)
    return b.getvalue()


def cases():
    """(name, kind, (H, W), class, save options)"""
    out = []
    variants = (("q75", "noise", dict(quality=75)), ("q20", "smooth", dict(quality=20)), ("q100", "edge", dict(quality=100)))
    for k, (H, W) in enumerate(SIZES):
        for cls in CLASSES:
            name, kind, kw = variants[(k + CLASSES.index(cls)) % 3]      # every size x class once, the variants rotating
            out.append((f"{H}x{W}_{cls}_{name}_{kind}", kind, (H, W), cls, kw))
    for cls in CLASSES:                                                   # crops and the end-to-end tests read these
        for H, W in ((33, 47), (64, 80)):
            out.append((f"{H}x{W}_{cls}_q90_noise", "noise", (H, W), cls, dict(quality=90)))
    for cls in CLASSES:
        out.append((f"33x47_{cls}_opt_noise", "noise", (33, 47), cls, dict(quality=75, optimize=True)))
        out.append((f"33x47_{cls}_rstblk_edge", "edge", (33, 47), cls, dict(quality=85, restart_marker_blocks=1)))
        out.append((f"64x80_{cls}_rstrow_smooth", "smooth", (64, 80), cls, dict(quality=60, restart_marker_rows=1)))
    out.append(("33x47_420_progressive", "noise", (33, 47), "420", dict(quality=75, progressive=True)))
    return out


def main():
    assert features.check_feature("libjpeg_turbo"), "the fixtures are libjpeg-turbo's output"
    data = {"pil_version": np.array(PIL.__version__), "jpeg_version": np.array(str(features.version("jpg"))),
            "libjpeg_turbo": np.array(bool(features.check_feature("libjpeg_turbo")))}
    names = []
    for k, (name, kind, (H, W), cls, kw) in enumerate(cases()):
        raw = encode(content(kind, H, W, k), cls, **kw)
        names.append(name)
        data["jpg_" + name] = np.frombuffer(raw, np.uint8)
        data["rgb_" + name] = np.asarray(Image.open(io.BytesIO(raw)).convert("RGB"))
    data["names"] = np.array(names)
    path = os.path.join(HERE, "jpeg_cases.npz")
    np.savez_compressed(path, **data)
    print(path, len(names), "cases", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
