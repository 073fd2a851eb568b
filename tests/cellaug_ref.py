"""numpy restatement of the device-side cell augmentation (include/fastvim_hip.h at fv_cellaug_geom): both launches and the
host's matrix and kernel construction, integer or fp32 in exactly the documented order.  OpenCV is not a dependency, so
this restatement is the contract; tests/test_cellaug_cpu.py ties it to scipy's independent fp64 arithmetic."""
import math

import numpy as np

NONE, HFLIP, VFLIP, ROTATE = 0, 1, 2, 3
TAPS = 9


def rotation_matrix(h, w, angle):
    """Inverse (destination to source) map of a rotation by ``angle`` degrees about ((w - 1) / 2, (h - 1) / 2):
    getRotationMatrix2D((w / 2 - 0.5, h / 2 - 0.5), angle, 1), then the closed-form affine inverse."""
    cx, cy = w / 2 - 0.5, h / 2 - 0.5
    rad = angle * (math.pi / 180.0)
    alpha, beta = math.cos(rad), math.sin(rad)
    M = [alpha, beta, (1 - alpha) * cx - beta * cy, -beta, alpha, beta * cx + (1 - alpha) * cy]
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[4] * D, M[0] * D
    M[0] = A11
    M[1] *= -D
    M[3] *= -D
    M[4] = A22
    b1 = -M[0] * M[2] - M[1] * M[5]
    b2 = -M[3] * M[2] - M[4] * M[5]
    M[2], M[5] = b1, b2
    return tuple(M)


def defocus_kernel_full(radius, sigma):
    """17 x 17: the disk (X^2 + Y^2 <= r^2) / count blurred by a separable 3-tap Gaussian of ``sigma``, fp32, rows first."""
    n = max(8, radius)
    size = 2 * n + 1
    disk = np.zeros((size, size), np.float32)
    for y in range(size):
        for x in range(size):
            if (x - n) ** 2 + (y - n) ** 2 <= radius ** 2:
                disk[y, x] = 1
    disk = disk / np.float32(disk.sum(dtype=np.float32))
    gs = np.exp(-np.array([1.0, 0.0, 1.0]) / (2.0 * sigma * sigma))
    g = (gs / gs.sum()).astype(np.float32)

    def blur_rows(a):
        out = np.zeros_like(a)
        for x in range(size):
            left = a[:, x - 1] if x > 0 else np.zeros(size, np.float32)
            right = a[:, x + 1] if x + 1 < size else np.zeros(size, np.float32)
            out[:, x] = np.float32(left * g[0] + a[:, x] * g[1]) + right * g[2]
        return out

    return np.ascontiguousarray(blur_rows(blur_rows(disk).T).T)


def defocus_kernel(radius, sigma):
    k = defocus_kernel_full(radius, sigma)
    c = k.shape[0] // 2
    return np.ascontiguousarray(k[c - 4:c + 5, c - 4:c + 5])


def reflect101(i, n):
    """BORDER_REFLECT_101 / numpy 'reflect' / scipy 'mirror' for any integer index."""
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i < n, i, p - i)


def _rint(v):
    return np.rint(v).astype(np.int64)


def warp_taps(h, w, m):
    """The fixed-point bilinear scheme on an h x w destination: four (row, col) tap index arrays, reflected within
    h x w, and the four integer weights (they sum to 32768)."""
    m0, m1, m2, m3, m4, m5 = (np.float64(v) for v in m)
    x = np.arange(w, dtype=np.float64)[None, :]
    y = np.arange(h, dtype=np.float64)[:, None]
    adelta, bdelta = _rint(m0 * x * 1024.0), _rint(m3 * x * 1024.0)
    X0, Y0 = _rint((m1 * y + m2) * 1024.0) + 16, _rint((m4 * y + m5) * 1024.0) + 16
    X, Y = (X0 + adelta) >> 5, (Y0 + bdelta) >> 5
    sx, fx, sy, fy = X >> 5, X & 31, Y >> 5, Y & 31
    rows = [reflect101(sy, h), reflect101(sy, h), reflect101(sy + 1, h), reflect101(sy + 1, h)]
    cols = [reflect101(sx, w), reflect101(sx + 1, w), reflect101(sx, w), reflect101(sx + 1, w)]
    weights = [(32 - fy) * (32 - fx) * 32, (32 - fy) * fx * 32, fy * (32 - fx) * 32, fy * fx * 32]
    return rows, cols, weights


def warp(img, m):
    """Rotate a (..., h, w) uint8 array by the inverse matrix ``m``."""
    h, w = img.shape[-2:]
    rows, cols, weights = warp_taps(h, w, m)
    acc = np.zeros(img.shape, np.int64)
    for r, c, wt in zip(rows, cols, weights):
        acc += img[..., r, c].astype(np.int64) * wt
    return ((acc + 16384) >> 15).astype(np.uint8)


def _lookup(src, oy, ox, rows, cols):
    """crop[c][row][col] = src[c][row - oy][col - ox] inside the source, 0 outside."""
    c, h, w = src.shape
    sy, sx = rows - oy, cols - ox
    inside = (sy >= 0) & (sy < h) & (sx >= 0) & (sx < w)
    v = src[:, np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)]
    return np.where(inside[None], v, 0).astype(np.uint8)


def geom(src, size, oy, ox, op=NONE, matrix=None):
    """fv_cellaug_geom for one sample: (C, H, W) uint8 -> (C, S, S) uint8."""
    S = size
    yy, xx = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    if op == HFLIP:
        xx = S - 1 - xx
    elif op == VFLIP:
        yy = S - 1 - yy
    if op != ROTATE:
        return _lookup(src, oy, ox, yy, xx)
    rows, cols, weights = warp_taps(S, S, matrix)
    acc = np.zeros((src.shape[0], S, S), np.int64)
    for r, c, wt in zip(rows, cols, weights):
        acc += _lookup(src, oy, ox, r, c).astype(np.int64) * wt
    return ((acc + 16384) >> 15).astype(np.uint8)


def correlate(planes, kernel):
    """Defocus of (..., h, w) uint8 planes: fp32, taps in row-major order, exact zeros skipped, one rounded product and one
    rounded add per tap, reflect-101 borders, rint, clamp."""
    kernel = np.asarray(kernel, np.float32)
    kh, kw = kernel.shape
    h, w = planes.shape[-2:]
    pad = [(0, 0)] * (planes.ndim - 2) + [(kh // 2, kh // 2), (kw // 2, kw // 2)]
    p = np.pad(planes, pad, mode="reflect").astype(np.float32)
    acc = np.zeros(planes.shape, np.float32)
    for ky in range(kh):
        for kx in range(kw):
            wt = kernel[ky, kx]
            if wt == 0:
                continue
            t = (p[..., ky:ky + h, kx:kx + w] * wt).astype(np.float32)
            acc = (acc + t).astype(np.float32)
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def filter(planes, kernel=None, holes=()):
    """fv_cellaug_filter for one sample: (C, S, S) uint8 -> (C, S, S) uint8."""
    out = correlate(planes, kernel) if kernel is not None else planes.copy()
    for y1, x1, y2, x2 in holes:
        out[:, y1:y2, x1:x2] = 0
    return out


def apply(src, size, plan):
    """Both launches for one sample and a ``fastvim_amd.cellaug.CellPlan``-like object (or ``None``: the identity)."""
    if plan is None:
        return src.copy()
    m = rotation_matrix(size, size, plan.angle) if plan.op == ROTATE else None
    g = geom(src, size, plan.oy, plan.ox, plan.op, m)
    return filter(g, defocus_kernel(plan.radius, plan.sigma) if plan.radius > 0 else None, plan.holes)
