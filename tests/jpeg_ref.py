"""A numpy restatement of baseline JPEG decoding as libjpeg-turbo (and so PIL) computes it: marker parser, Huffman
decoder, dequantisation + the ``jidctint`` "islow" 8 x 8 inverse DCT, fancy chroma upsampling over the TRUE plane sizes and
the ``jdcolor`` YCbCr -> RGB conversion.  tests/test_jpeg_cpu.py holds it to PIL (live, and PIL-written fixtures); the C++
entropy decoder and the HIP kernels of fastvim_amd/jpeg.py are held to it.

The served class, as ``fv_jpeg_probe`` states it: SOF0, 8 bits, one interleaved scan, 8-bit tables; one component, or three
read as YCbCr with luma sampling 1x1 / 2x1 / 2x2 and chroma 1x1."""
import numpy as np

S444, S422, S420, GRAY = 0, 1, 2, 3
(OK, PROGRESSIVE, ARITHMETIC, PRECISION, COMPONENTS, COLOUR, SAMPLING, SCANS, TABLES16, MALFORMED, FRAME) = range(11)
REASONS = ("served", "progressive", "arithmetic coding", "not 8-bit precision", "not 1 or 3 components",
           "not YCbCr (Adobe transform 0 or RGB component ids)", "sampling factors", "several scans",
           "16-bit quantisation tables", "malformed or not a JPEG", "frame type other than SOF0")

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                   60, 61, 54, 47, 55, 62, 63])          # natural index of the k-th coefficient in file order


class Unserved(Exception):
    def __init__(self, reason, H=0, W=0, ncomp=0):
        super().__init__(REASONS[reason])
        self.reason, self.H, self.W, self.ncomp = reason, H, W, ncomp


class DecodeError(Exception):
    pass


class Header:
    pass


# --------------------------------------------------------------------------------------------------------------- parser
def parse(data):
    """Markers up to and including the first SOS.  Raises ``Unserved``."""
    d = bytes(data)
    n = len(d)
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise Unserved(MALFORMED)
    hd = Header()
    hd.qt, hd.qt16, hd.huff, hd.ri, hd.adobe, hd.jfif, hd.frame = {}, False, {}, 0, None, False, None
    pos = 2
    while True:
        if pos + 4 > n or d[pos] != 0xFF:
            raise Unserved(MALFORMED)
        while pos + 1 < n and d[pos + 1] == 0xFF:
            pos += 1
        m = d[pos + 1]
        pos += 2
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9 or pos + 2 > n:
            raise Unserved(MALFORMED)
        ln = (d[pos] << 8) | d[pos + 1]
        if ln < 2 or pos + ln > n:
            raise Unserved(MALFORMED)
        seg = d[pos + 2:pos + ln]
        pos += ln
        if m == 0xDB:
            q = 0
            while q < len(seg):
                pq, tq = seg[q] >> 4, seg[q] & 15
                if tq > 3 or pq > 1 or q + 1 + 64 * (pq + 1) > len(seg):
                    raise Unserved(MALFORMED)
                if pq:
                    vals = [(seg[q + 1 + 2 * k] << 8) | seg[q + 2 + 2 * k] for k in range(64)]
                else:
                    vals = list(seg[q + 1:q + 65])
                t = np.zeros(64, np.int32)
                t[ZIGZAG] = vals
                hd.qt[tq] = (t, bool(pq))
                q += 1 + 64 * (pq + 1)
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                if q + 17 > len(seg):
                    raise Unserved(MALFORMED)
                tc, th = seg[q] >> 4, seg[q] & 15
                counts = list(seg[q + 1:q + 17])
                nv = sum(counts)
                if tc > 1 or th > 3 or nv > 256 or q + 17 + nv > len(seg):
                    raise Unserved(MALFORMED)
                hd.huff[(tc, th)] = _huff(counts, list(seg[q + 17:q + 17 + nv]))
                q += 17 + nv
        elif m == 0xDD:
            if len(seg) != 2:
                raise Unserved(MALFORMED)
            hd.ri = (seg[0] << 8) | seg[1]
        elif m == 0xE0 and len(seg) >= 14 and seg[:5] == b"JFIF\0":
            hd.jfif = True
        elif m == 0xEE and len(seg) >= 12 and seg[:5] == b"Adobe":
            hd.adobe = seg[11]
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            if hd.frame is not None or len(seg) < 6:
                raise Unserved(MALFORMED)
            hd.frame, hd.precision = m, seg[0]
            hd.H, hd.W, nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if len(seg) != 6 + 3 * nc or hd.H == 0 or hd.W == 0 or nc == 0:
                raise Unserved(MALFORMED)
            hd.comps = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(nc)]
        elif m == 0xDA:
            if hd.frame is None:
                raise Unserved(MALFORMED)
            _classify(hd, seg)
            hd.scan = pos
            return hd


def _classify(hd, sos):
    H, W, nc = hd.H, hd.W, len(hd.comps)

    def no(r):
        raise Unserved(r, H, W, nc)
    if hd.frame in (0xC2, 0xC6, 0xCA, 0xCE):
        no(PROGRESSIVE)
    if hd.frame >= 0xC9:
        no(ARITHMETIC)
    if hd.frame != 0xC0:
        no(FRAME)
    if hd.precision != 8:
        no(PRECISION)
    if nc not in (1, 3):
        no(COMPONENTS)
    if nc == 3:
        ids = bytes(c[0] for c in hd.comps)
        if hd.adobe is not None:
            if hd.adobe != 1:
                no(COLOUR)
        elif not hd.jfif and ids == b"RGB":
            no(COLOUR)
    hv = [(c[1], c[2]) for c in hd.comps]
    if any(not (1 <= h <= 4 and 1 <= v <= 4) for h, v in hv):
        no(MALFORMED)
    if nc == 1:
        if hv[0] != (1, 1):
            no(SAMPLING)
        hd.cls = GRAY
    else:
        if hv[1] != (1, 1) or hv[2] != (1, 1) or hv[0] not in ((1, 1), (2, 1), (2, 2)):
            no(SAMPLING)
        hd.cls = {(1, 1): S444, (2, 1): S422, (2, 2): S420}[hv[0]]
    if len(sos) < 1 or len(sos) != 4 + 2 * sos[0]:
        no(MALFORMED)
    if sos[0] != nc:
        no(SCANS)
    hd.tabs = []
    for c in range(nc):
        if sos[1 + 2 * c] != hd.comps[c][0]:
            no(SCANS)
        td, ta = sos[2 + 2 * c] >> 4, sos[2 + 2 * c] & 15
        if (0, td) not in hd.huff or (1, ta) not in hd.huff or hd.comps[c][3] not in hd.qt:
            no(MALFORMED)
        if hd.qt[hd.comps[c][3]][1]:
            no(TABLES16)
        hd.tabs.append((td, ta))
    if sos[1 + 2 * nc] != 0 or sos[2 + 2 * nc] != 63 or sos[3 + 2 * nc] != 0:
        no(MALFORMED)
    hd.hmax, hd.vmax = hv[0]
    hd.mcus_x = -(-W // (8 * hd.hmax))
    hd.mcus_y = -(-H // (8 * hd.vmax))


def probe(data):
    """(height, width, components, sampling class, served, reason)."""
    try:
        hd = parse(data)
    except Unserved as e:
        return e.H, e.W, e.ncomp, -1, False, e.reason
    return hd.H, hd.W, len(hd.comps), hd.cls, True, OK


def mcu_window(H, W, cls, crop=None):
    """The MCU rectangle (x0, y0, w, h) a crop (top, left, h, w) needs: the crop widened by 2 luma pixels where chroma is
    subsampled, clamped to the image, widened to whole MCUs."""
    hmax, vmax = ((1, 1), (2, 1), (2, 2), (1, 1))[cls]
    t, l, h, w = (0, 0, H, W) if crop is None else crop
    px, py = 2 * (hmax > 1), 2 * (vmax > 1)
    x0, x1 = max(l - px, 0), min(l + w + px, W)
    y0, y1 = max(t - py, 0), min(t + h + py, H)
    mw, mh = 8 * hmax, 8 * vmax
    return x0 // mw, y0 // mh, -(-x1 // mw) - x0 // mw, -(-y1 // mh) - y0 // mh


# -------------------------------------------------------------------------------------------------------------- Huffman
def _huff(counts, vals):
    """code -> symbol as a dict keyed by (length, code)."""
    table, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(counts[ln - 1]):
            if code >= 1 << ln:
                raise Unserved(MALFORMED)
            table[(ln, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return table


class _Bits:
    def __init__(self, d, pos):
        self.d, self.pos, self.acc, self.n = d, pos, 0, 0

    def bit(self):
        if self.n == 0:
            d, p = self.d, self.pos
            if p >= len(d):
                raise DecodeError("data ends early")
            b = d[p]
            if b == 0xFF:
                while p + 1 < len(d) and d[p + 1] == 0xFF:
                    p += 1
                if p + 1 >= len(d) or d[p + 1] != 0:
                    raise DecodeError("data ends early (marker)")
                p += 1
            self.pos, self.acc, self.n = p + 1, b, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def get(self, s):
        v = 0
        for _ in range(s):
            v = (v << 1) | self.bit()
        return v

    def sym(self, table):
        code = 0
        for ln in range(1, 17):
            code = (code << 1) | self.bit()
            s = table.get((ln, code))
            if s is not None:
                return s
        raise DecodeError("bad Huffman code")

    def restart(self, k):
        d, p = self.d, self.pos
        self.n = 0
        if p + 1 >= len(d) or d[p] != 0xFF:
            raise DecodeError("restart marker missing")
        while p + 1 < len(d) and d[p + 1] == 0xFF:
            p += 1
        if p + 1 >= len(d) or d[p + 1] != 0xD0 + (k & 7):
            raise DecodeError("wrong restart marker")
        self.pos = p + 2


def _extend(v, s):
    return v if v >= (1 << (s - 1)) else v - (1 << s) + 1


def entropy_decode(data, window=None):
    """-> (header, [per component (block rows, block cols, 64) int16, natural order], MCUs decoded).  ``window`` is an MCU
    rectangle (x0, y0, w, h); decoding stops after the last MCU it needs."""
    hd = parse(data)
    d = bytes(data)
    nc = len(hd.comps)
    x0, y0, mw, mh = (0, 0, hd.mcus_x, hd.mcus_y) if window is None else window
    if not (0 <= x0 and 0 <= y0 and mw >= 1 and mh >= 1 and x0 + mw <= hd.mcus_x and y0 + mh <= hd.mcus_y):
        raise ValueError("window outside the image")
    hv = [(c[1], c[2]) for c in hd.comps] if nc == 3 else [(1, 1)]
    coefs = [np.zeros((mh * v, mw * h, 64), np.int16) for h, v in hv]
    bits, pred = _Bits(d, hd.scan), [0] * nc
    last = (y0 + mh - 1) * hd.mcus_x + x0 + mw - 1
    for m in range(last + 1):
        if hd.ri and m and m % hd.ri == 0:
            bits.restart(m // hd.ri - 1)
            pred = [0] * nc
        my, mx = divmod(m, hd.mcus_x)
        inside = y0 <= my < y0 + mh and x0 <= mx < x0 + mw
        for c in range(nc):
            dc, ac = hd.huff[(0, hd.tabs[c][0])], hd.huff[(1, hd.tabs[c][1])]
            h, v = hv[c]
            for by in range(v):
                for bx in range(h):
                    blk = np.zeros(64, np.int16)
                    s = bits.sym(dc)
                    if s > 15:
                        raise DecodeError("bad DC size")
                    if s:
                        pred[c] += _extend(bits.get(s), s)
                    blk[0] = np.int64(pred[c]).astype(np.int16)
                    k = 1
                    while k < 64:
                        rs = bits.sym(ac)
                        r, s = rs >> 4, rs & 15
                        if s:
                            k += r
                            if k > 63:
                                raise DecodeError("run past 63")
                            blk[ZIGZAG[k]] = _extend(bits.get(s), s)
                            k += 1
                        elif r == 15:
                            k += 16
                            if k > 64:
                                raise DecodeError("run past 63")
                        else:
                            break
                    if inside:
                        coefs[c][(my - y0) * v + by, (mx - x0) * h + bx] = blk
    return hd, coefs, last + 1


def qtables(hd):
    return [hd.qt[c[3]][0] for c in hd.comps]


# ----------------------------------------------------------------------------------------------------------------- IDCT
def idct(coef):
    """(..., 64) dequantised int32, natural order -> (..., 8, 8) uint8: jidctint islow, columns first."""
    a = np.asarray(coef, np.int64).reshape(coef.shape[:-1] + (8, 8))

    def pass_(x, axis, shift):
        i = [np.take(x, k, axis=axis) for k in range(8)]
        z1 = (i[2] + i[6]) * 4433
        tmp2 = z1 - i[6] * 15137
        tmp3 = z1 + i[2] * 6270
        tmp0 = (i[0] + i[4]) << 13
        tmp1 = (i[0] - i[4]) << 13
        tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
        t0, t1, t2, t3 = i[7], i[5], i[3], i[1]
        z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
        z5 = (z3 + z4) * 9633
        t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
        z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
        t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
        o = [tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3]
        return np.stack([(v + (1 << (shift - 1))) >> shift for v in o], axis=axis)

    a = pass_(a, -2, 11)          # columns: the index along a column is the ROW axis
    a = pass_(a, -1, 18)
    return np.clip(a + 128, 0, 255).astype(np.uint8)


def planes(hd, coefs):
    """The window-local sample planes, one per component: (block rows * 8, block cols * 8) uint8."""
    out = []
    for c, q in zip(coefs, qtables(hd)):
        px = idct(c.astype(np.int32) * q)                             # (bh, bw, 8, 8)
        out.append(px.transpose(0, 2, 1, 3).reshape(c.shape[0] * 8, c.shape[1] * 8))
    return out


# -------------------------------------------------------------------------------------------------- upsampling + colour
def _fix(x):
    return int(x * 65536 + 0.5)


def to_rgb(hd, pl, window, crop=None):
    """The crop (top, left, h, w) of the image as (h, w, 3) uint8, from the window-local planes."""
    H, W, cls = hd.H, hd.W, hd.cls
    t, l, h, w = (0, 0, H, W) if crop is None else crop
    x0, y0 = window[0], window[1]
    Y = (t + np.arange(h))[:, None]
    X = (l + np.arange(w))[None, :]
    lum = pl[0][Y - y0 * 8 * hd.vmax, X - x0 * 8 * hd.hmax].astype(np.int64)
    if cls == GRAY:
        return np.repeat(lum[:, :, None], 3, axis=2).astype(np.uint8)
    cw, ch = -(-W // hd.hmax), -(-H // hd.vmax)
    cx, cy = X // hd.hmax, Y // hd.vmax
    chroma = []
    for p in pl[1:]:
        def at(yy, xx):
            return p[np.clip(yy, 0, ch - 1) - y0 * 8, np.clip(xx, 0, cw - 1) - x0 * 8].astype(np.int64)
        if cls == S444:
            v = at(cy, cx)
        elif cls == S422:
            nb = np.where(X % 2 == 0, cx - 1, cx + 1)
            v = (3 * at(cy, cx) + at(cy, nb) + np.where(X % 2 == 0, 1, 2)) >> 2
        else:
            ny = np.where(Y % 2 == 0, cy - 1, cy + 1)
            nx = np.where(X % 2 == 0, cx - 1, cx + 1)
            here = 3 * at(cy, cx) + at(ny, cx)
            there = 3 * at(cy, nx) + at(ny, nx)
            v = (3 * here + there + np.where(X % 2 == 0, 8, 7)) >> 4
        chroma.append(v - 128)
    cb, cr = chroma
    r = lum + ((_fix(1.402) * cr + 32768) >> 16)
    g = lum + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    b = lum + ((_fix(1.772) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def decode(data, crop=None):
    """The RGB image (or its crop) as PIL's ``Image.open(...).convert("RGB")`` gives it, through the MCU window of the crop."""
    hd = parse(data)
    win = mcu_window(hd.H, hd.W, hd.cls, crop)
    hd, coefs, _ = entropy_decode(data, win)
    return to_rgb(hd, planes(hd, coefs), win, crop)
