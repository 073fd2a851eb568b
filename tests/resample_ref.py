"""Numpy restatement of PIL's 8-bit bicubic resize (``ImagingResample``: horizontal pass, uint8 intermediate, vertical pass,
integer coefficients of 22 fraction bits) followed by a crop window and a horizontal flip -- the reference of
``fastvim_amd.resample`` / csrc/resample.hip.  Test infrastructure: the product does not import it.

Per axis, input length ``n``, output length ``m``, all in fp64 (numpy scalars: IEEE operations, no contraction):
``scale = n / m``, ``fs = max(scale, 1)``, ``support = 2 fs``; for output ``i``: ``center = (i + 0.5) scale``, ``lo =
max(int(center - support + 0.5), 0)``, ``hi = min(int(center + support + 0.5), n)``, ``w_k = bicubic((k + lo - center + 0.5)
(1 / fs))``, normalised by their sum taken in ascending ``k`` (when it is not 0), and ``c_k = int(w_k 2^22 +- 0.5)``
truncated toward zero.  One output value: ``clip((2^21 + sum_k src[lo + k] c_k) >> 22, 0, 255)`` in int32."""
import numpy as np

PRECISION_BITS = 22


def bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(n, m, first=0, count=None):
    """``(lo, cnt, c)`` for outputs ``first .. first + count - 1`` of an ``n -> m`` resize: int arrays ``lo``, ``cnt`` of
    ``count`` entries and ``c`` (count, max cnt) int64, zero past ``cnt``."""
    count = m - first if count is None else count
    scale = float(n) / float(m)
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ss = 1.0 / fs
    los, cnts, rows = [], [], []
    for i in range(first, first + count):
        center = (i + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), n)
        cnt = hi - lo
        w = [bicubic((k + lo - center + 0.5) * ss) for k in range(cnt)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        rows.append([int(0.5 + v * (1 << PRECISION_BITS)) if v >= 0 else int(-0.5 + v * (1 << PRECISION_BITS)) for v in w])
        los.append(lo)
        cnts.append(cnt)
    c = np.zeros((count, max(cnts + [1])), np.int64)
    for i, r in enumerate(rows):
        c[i, :len(r)] = r
    return np.array(los), np.array(cnts), c


def _pass(src, lo, cnt, c):
    """Resample axis 0 of ``src`` (n, ...) uint8 -> (len(lo), ...) uint8."""
    out = np.empty((len(lo),) + src.shape[1:], np.uint8)
    s = src.astype(np.int64)
    for i in range(len(lo)):
        acc = np.tensordot(c[i, :cnt[i]], s[lo[i]:lo[i] + cnt[i]], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        acc = ((acc + (1 << 31)) % (1 << 32)) - (1 << 31)          # int32 wrap-around, as the C accumulator
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize(a, o_h, o_w, window=None):
    """``a`` (H, W, C) uint8 -> the ``(win_y, win_x, s_h, s_w)`` window (default: all) of its bicubic resize to
    ``o_h x o_w``, (s_h, s_w, C) uint8."""
    a = np.asarray(a)
    H, W = a.shape[:2]
    wy, wx, sh, sw = (0, 0, o_h, o_w) if window is None else window
    assert 0 <= wy and wy + sh <= o_h and 0 <= wx and wx + sw <= o_w
    lx, cx, kx = coeffs(W, o_w, wx, sw)
    ly, cy, ky = coeffs(H, o_h, wy, sh)
    r0, r1 = int(ly.min()), int((ly + cy).max())                 # the source rows the window needs
    tmp = _pass(np.ascontiguousarray(a[r0:r1].transpose(1, 0, 2)), lx, cx, kx).transpose(1, 0, 2)      # (rows, s_w, C)
    return _pass(tmp, ly - r0, cy, ky)


def resample(a, crop=None, out_full=None, window=(0, 0), size=None, flip=False):
    """One sample of ``ImageStage``: crop ``(i, j, h, w)`` of ``a`` (H, W, 3), resized to ``out_full = (o_h, o_w)``
    (default: ``size``), the ``size = (s_h, s_w)`` window at ``window``, mirrored if ``flip``; planar (3, s_h, s_w) uint8."""
    a = np.asarray(a)
    if crop is not None:
        i, j, h, w = crop
        a = a[i:i + h, j:j + w]
    size = out_full if size is None else size
    o_h, o_w = size if out_full is None else out_full
    r = resize(a, o_h, o_w, (window[0], window[1], size[0], size[1]))
    if flip:
        r = r[:, ::-1]
    return np.ascontiguousarray(r.transpose(2, 0, 1))
