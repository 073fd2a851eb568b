"""Numpy restatement of the pixel operations of timm's RandAugment as PIL computes them on 8-bit RGB images (the contract
of csrc/randaug.hip; held to PIL itself and to PIL-written fixtures by tests/test_randaug_cpu.py).  Plain Python: no HIP
library, no torch.  Images are (H, W, 3) uint8 arrays; ``apply_record`` / ``apply_plan`` take the records that
``fastvim_amd.randaug.RandAugment`` draws (``Record``: kind, two ints, the blend factor, the fill colour, six doubles).

Every float operation below is written in the order PIL's C code performs it: float32 for ``Image.blend`` and the 3x3
filter, float64 for the affine warp; nothing is contracted or reassociated by numpy."""
import numpy as np

# the kinds of include/fastvim_hip.h (FV_RA_*)
COPY, AUTOCONTRAST, EQUALIZE, INVERT, SOLARIZE, POSTERIZE, SOLARIZE_ADD, COLOR, CONTRAST, BRIGHTNESS, SHARPNESS, AFFINE = range(12)

_IDENT = np.arange(256, dtype=np.int64)


def histogram(a):
    """(3, 256) counts of an (H, W, 3) uint8 image."""
    return np.stack([np.bincount(a[..., c].reshape(-1), minlength=256) for c in range(3)])


def autocontrast_lut(h):
    """``ImageOps.autocontrast(img)`` (cutoff 0) of one channel's histogram ``h``: (256,) table."""
    nz = np.nonzero(h)[0]
    if len(nz) == 0 or nz[-1] <= nz[0]:
        return _IDENT.copy()
    lo, hi = int(nz[0]), int(nz[-1])
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.clip(np.trunc(np.arange(256, dtype=np.float64) * scale + offset), 0, 255).astype(np.int64)


def equalize_lut(h):
    """``ImageOps.equalize(img)`` of one channel's histogram: integers only; entries above 255 are CLIPPED (``Image.point``)."""
    histo = [int(v) for v in h if v]
    if len(histo) <= 1:
        return _IDENT.copy()
    step = (sum(histo) - histo[-1]) // 255
    if step == 0:
        return _IDENT.copy()
    n, lut = step // 2, []
    for i in range(256):
        lut.append(min(n // step, 255))
        n += int(h[i])
    return np.array(lut, np.int64)


def fixed_lut(kind, arg0=0, arg1=0):
    i = _IDENT
    if kind == INVERT:
        return 255 - i
    if kind == SOLARIZE:
        return np.where(i < arg0, i, 255 - i)
    if kind == POSTERIZE:
        return i & ~(2 ** (8 - arg0) - 1)
    if kind == SOLARIZE_ADD:
        return np.where(i < arg1, np.minimum(255, i + arg0), i)
    raise ValueError(kind)


def point(a, luts):
    """``luts``: (256,) for all channels or (3, 256)."""
    luts = np.broadcast_to(np.asarray(luts), (3, 256))
    return np.stack([luts[c][a[..., c]] for c in range(3)], axis=-1).astype(np.uint8)


def _clip8(t):
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.uint8)


def blend(d, a, factor):
    """``Image.blend(degenerate, image, factor)``: ``d`` and ``a`` integer arrays of one shape."""
    alpha = np.float32(factor)
    d, a = np.asarray(d, np.int32), np.asarray(a, np.int32)
    if alpha == 0:
        return d.astype(np.uint8)
    if alpha == 1:
        return a.astype(np.uint8)
    t = d.astype(np.float32) + alpha * (a - d).astype(np.float32)
    assert t.dtype == np.float32
    if 0 <= alpha <= 1:
        return np.trunc(t).astype(np.uint8)
    return _clip8(t)


def grey(a):
    a = a.astype(np.int64)
    return (a[..., 0] * 19595 + a[..., 1] * 38470 + a[..., 2] * 7471 + 0x8000) >> 16


def contrast_mean(a):
    g = grey(a)
    return int(float(int(g.sum())) / float(g.size) + 0.5)


def smooth(a):
    """``ImageFilter.SMOOTH``: borders copied; float32 weights k / 13, accumulator from 0.5, rows y + 1, y, y - 1."""
    H, W = a.shape[:2]
    out = a.copy()
    if H < 3 or W < 3:
        return out
    k = np.array([1, 1, 1, 1, 5, 1, 1, 1, 1], np.float32) / np.float32(13)
    p = a.astype(np.float32)
    acc = np.full((H - 2, W - 2, 3), 0.5, np.float32)
    for r, ys in enumerate((slice(2, H), slice(1, H - 1), slice(0, H - 2))):
        row = p[ys]
        part = row[:, 0:W - 2] * k[3 * r] + row[:, 1:W - 1] * k[3 * r + 1]
        part = part + row[:, 2:W] * k[3 * r + 2]
        acc = acc + part
    assert acc.dtype == np.float32
    out[1:H - 1, 1:W - 1] = _clip8(acc)
    return out


def _cubic(v1, v2, v3, v4, d):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def affine(a, m, fill):
    """``img.transform(img.size, Image.AFFINE, m, Image.BICUBIC, fillcolor=fill)``, fp64."""
    H, W = a.shape[:2]
    m = [float(v) for v in m]
    x = np.arange(W, dtype=np.float64)[None, :] + 0.5
    y = np.arange(H, dtype=np.float64)[:, None] + 0.5
    xin = m[0] * x + m[1] * y + m[2]
    yin = m[3] * x + m[4] * y + m[5]
    outside = ~((xin >= 0) & (xin < W) & (yin >= 0) & (yin < H))
    xin = np.where(outside, 0.5, xin) - 0.5
    yin = np.where(outside, 0.5, yin) - 0.5
    xf, yf = np.floor(xin), np.floor(yin)
    dx, dy = xin - xf, yin - yf
    x0, y0 = xf.astype(np.int64) - 1, yf.astype(np.int64) - 1
    xs = [np.clip(x0 + k, 0, W - 1) for k in range(4)]
    p = a.astype(np.float64)
    out = np.empty_like(a)
    for c in range(3):
        pc = p[..., c]
        rows = []
        for k in range(4):
            yk = y0 + k
            v = _cubic(*(pc[np.clip(yk, 0, H - 1), xs[j]] for j in range(4)), dx)
            if k > 0:
                v = np.where((yk >= 0) & (yk < H), v, rows[-1])
            rows.append(v)
        v = _cubic(rows[0], rows[1], rows[2], rows[3], dy)
        out[..., c] = np.where(outside, fill[c], _clip8(v))
    return out


def apply_record(a, rec):
    """One layer: ``rec`` has .kind, .arg0, .arg1, .factor, .fill (three ints) and .coeffs (six floats)."""
    k = rec.kind
    if k == COPY:
        return a.copy()
    if k == AUTOCONTRAST:
        return point(a, np.stack([autocontrast_lut(h) for h in histogram(a)]))
    if k == EQUALIZE:
        return point(a, np.stack([equalize_lut(h) for h in histogram(a)]))
    if k in (INVERT, SOLARIZE, POSTERIZE, SOLARIZE_ADD):
        return point(a, fixed_lut(k, rec.arg0, rec.arg1))
    if k == COLOR:
        return blend(np.repeat(grey(a)[..., None], 3, axis=-1), a, rec.factor)
    if k == CONTRAST:
        return blend(np.full(a.shape, contrast_mean(a)), a, rec.factor)
    if k == BRIGHTNESS:
        return blend(np.zeros(a.shape, np.int32), a, rec.factor)
    if k == SHARPNESS:
        return blend(smooth(a), a, rec.factor)
    if k == AFFINE:
        return affine(a, rec.coeffs, rec.fill)
    raise ValueError(f"unknown kind {k}")


def apply_plan(a, records):
    """The layers of one sample in order on an (H, W, 3) uint8 image."""
    for rec in records:
        a = apply_record(a, rec)
    return a


def equalize_overflow_image(H=224, W=224):
    """A random image whose equalize table reaches 256 before the clip in every channel (``Image.point`` clips, it does
    not wrap): the first seed for which ``(step // 2 + count below 255) // step >= 256`` holds."""
    for seed in range(64):
        a = np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
        ok = True
        for h in histogram(a):
            step = (int(h.sum()) - int(h[np.nonzero(h)[0][-1]])) // 255
            ok = ok and step > 0 and (step // 2 + int(h[:255].sum())) // step >= 256
        if ok:
            return a
    raise AssertionError("no seed found")
