"""A numpy restatement of the JPEG index (include/fastvim_hip.h at THE INDEX) and of "decode one group from its entry",
built on tests/jpeg_ref.py: the header words, the four Huffman tables in the form the device reads, one entry per group of
``S`` MCUs and the end sentinel.  The reader here works a bit at a time on a (byte, bit) cursor over the stuffed stream --
nothing is read ahead, so the cursor IS the position an entry records.  tests/test_jpeg_index_cpu.py holds the C++
builder to ``build_index`` byte for byte, and every group decoded on its own to ``jpeg_ref.entropy_decode``."""
import numpy as np

import jpeg_ref as R

MAGIC, VERSION, HEAD_WORDS, TABLE_WORDS, LOOK = 0x58494A46, 1, 224, 356, 9
ENTRIES = 4 * (HEAD_WORDS + 4 * TABLE_WORDS)          # byte offset of the first entry: 6592
RESTART, CHROMA_TABLES = "restart interval", "different Huffman tables for the two chroma components"


class NotIndexed(Exception):
    pass


def fnv1a(data):
    h = 0xcbf29ce484222325
    for b in bytes(data):
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h


def device_table(table):
    """One Huffman table of jpeg_ref (``{(length, code): symbol}``) as the 356 words the device reads."""
    t = np.zeros(TABLE_WORDS, np.uint32)
    look, maxcode, valoff = t[:256].view(np.uint16), t[256:274].view(np.int32), t[274:291].view(np.int32)
    vals = t[292:356].view(np.uint8)
    maxcode[:] = -1
    maxcode[17] = 0x7fffffff
    k, code = 0, 0
    for ln in range(1, 17):
        codes = sorted(c for (l, c) in table if l == ln)
        valoff[ln] = k - code                                      # the first code of a length that has none: as the walk leaves it
        for c in codes:
            assert c == code
            if ln <= LOOK:
                look[c << (LOOK - ln):(c + 1) << (LOOK - ln)] = ln << 8 | table[(ln, c)]
            vals[k] = table[(ln, c)]
            k, code = k + 1, code + 1
        if codes:
            maxcode[ln] = code - 1
        code <<= 1
    t[291] = k
    return t


class Cursor(R._Bits):
    """jpeg_ref's bit reader on a (byte, bit) cursor: a data 0xFF and its stuffed 0x00 are one step, a marker ends it."""

    def __init__(self, d, byte, bit):
        self.d, self.byte, self.at = d, byte, bit

    def bit(self):
        d, p = self.d, self.byte
        if p >= len(d):
            raise R.DecodeError("data ends early")
        b = d[p]
        if b == 0xFF and (p + 1 >= len(d) or d[p + 1] != 0):
            raise R.DecodeError("data ends early (marker)")
        v = (b >> (7 - self.at)) & 1
        self.at += 1
        if self.at == 8:
            self.at, self.byte = 0, p + (2 if b == 0xFF else 1)
        return v


def _block(bits, dc, ac, pred):
    """One block from the cursor: (natural-order int16 block, the new predictor)."""
    blk = np.zeros(64, np.int16)
    s = bits.sym(dc)
    if s > 15:
        raise R.DecodeError("bad DC size")
    if s:
        pred = int(np.int64(pred + R._extend(bits.get(s), s)).astype(np.int16))
    blk[0] = pred
    k = 1
    while k < 64:
        rs = bits.sym(ac)
        r, s = rs >> 4, rs & 15
        if s:
            k += r
            if k > 63:
                raise R.DecodeError("run past 63")
            blk[R.ZIGZAG[k]] = R._extend(bits.get(s), s)
            k += 1
        elif r == 15:
            k += 16
            if k > 64:
                raise R.DecodeError("run past 63")
        else:
            break
    return blk, pred


def _shape(hd):
    nc = len(hd.comps)
    return [(c[1], c[2]) for c in hd.comps] if nc == 3 else [(1, 1)]


def decode_group(d, hd, byte, bit, pred, count):
    """``count`` MCUs from the position (byte, bit) with the predictors ``pred``: ([per MCU {(c, by, bx): block}], the
    cursor behind them, the predictors behind them)."""
    bits, pred, out = Cursor(d, byte, bit), list(pred), []
    for _ in range(count):
        mcu = {}
        for c, (h, v) in enumerate(_shape(hd)):
            dc, ac = hd.huff[(0, hd.tabs[c][0])], hd.huff[(1, hd.tabs[c][1])]
            for by in range(v):
                for bx in range(h):
                    mcu[(c, by, bx)], pred[c] = _block(bits, dc, ac, pred[c])
        out.append(mcu)
    return out, (bits.byte, bits.at), pred


_WALKS = {}


def _walk(d, hd):
    """((byte, bit), predictors) in front of every MCU in file order, and behind the last: one pass, MCU after MCU, each
    started from where the one before ended (kept per file: an index of any S is a subset of it)."""
    if d not in _WALKS:
        pos, pred, out = (hd.scan, 0), [0] * len(hd.comps), []
        for _ in range(hd.mcus_x * hd.mcus_y):
            out.append((pos, list(pred)))
            _, pos, pred = decode_group(d, hd, pos[0], pos[1], pred, 1)
        out.append((pos, list(pred)))
        _WALKS[d] = out
    return _WALKS[d]


def build_index(data, S):
    """The index of ``data`` with groups of ``S`` MCUs, as bytes.  ``jpeg_ref.Unserved`` / ``NotIndexed`` with the reason."""
    d = bytes(data)
    hd = R.parse(d)
    if hd.ri:
        raise NotIndexed(RESTART)
    nc = len(hd.comps)
    if nc == 3 and hd.tabs[1] != hd.tabs[2]:
        raise NotIndexed(CHROMA_TABLES)
    gpr = -(-hd.mcus_x // S)
    groups = gpr * hd.mcus_y
    head = np.zeros(HEAD_WORDS, np.uint32)
    h = fnv1a(d)
    head[:15] = (MAGIC, VERSION, len(d) & 0xffffffff, len(d) >> 32, h & 0xffffffff, h >> 32, hd.H, hd.W, hd.cls, nc, hd.mcus_x,
                 hd.mcus_y, S, gpr, groups)
    head[16:18] = (hd.scan & 0xffffffff, hd.scan >> 32)
    for c, q in enumerate(R.qtables(hd)):
        head[32 + 64 * c:96 + 64 * c] = q
    cc = 1 if nc == 3 else 0
    tables = [device_table(hd.huff[k]) for k in ((0, hd.tabs[0][0]), (0, hd.tabs[cc][0]), (1, hd.tabs[0][1]), (1, hd.tabs[cc][1]))]
    walk = _walk(d, hd)
    entries = np.zeros((groups + 1, 4), np.uint32)
    for g in range(groups + 1):
        pos, pred = walk[(g // gpr) * hd.mcus_x + (g % gpr) * S] if g < groups else walk[-1]
        p = [int(np.int16(v).view(np.uint16)) for v in pred] + [0, 0]
        entries[g] = (pos[0], pos[1], p[0] | p[1] << 16, p[2])
    return np.concatenate([head, *tables, entries.reshape(-1)]).astype("<u4").tobytes()


def entries_of(index):
    w = np.frombuffer(index, "<u4")
    e = w[ENTRIES // 4:].reshape(-1, 4)
    preds = np.stack([(e[:, 2] & 0xffff).astype(np.uint16).view(np.int16), (e[:, 2] >> 16).astype(np.uint16).view(np.int16),
                      (e[:, 3] & 0xffff).astype(np.uint16).view(np.int16)], 1)
    return e[:, 0].astype(np.int64), e[:, 1].astype(np.int64), preds


def decode_window(data, index, window=None):
    """Every group that meets the MCU window ``(x0, y0, w, h)`` (default: the image) decoded ON ITS OWN from its entry:
    the window's coefficients per component, shaped as ``jpeg_ref.entropy_decode`` shapes them."""
    d = bytes(data)
    hd = R.parse(d)
    w = np.frombuffer(index, "<u4", 32)
    S, gpr = int(w[12]), int(w[13])
    byte, bit, preds = entries_of(index)
    x0, y0, mw, mh = (0, 0, hd.mcus_x, hd.mcus_y) if window is None else window
    hv = _shape(hd)
    coefs = [np.zeros((mh * v, mw * h, 64), np.int16) for h, v in hv]
    for my in range(y0, y0 + mh):
        for gx in range(x0 // S, (x0 + mw - 1) // S + 1):
            g = my * gpr + gx
            mcus, _, _ = decode_group(d, hd, int(byte[g]), int(bit[g]), [int(v) for v in preds[g][:len(hv)]],
                                      min(S, hd.mcus_x - gx * S))
            for k, mcu in enumerate(mcus):
                mx = gx * S + k
                if x0 <= mx < x0 + mw:
                    for (c, by, bx), blk in mcu.items():
                        coefs[c][(my - y0) * hv[c][1] + by, (mx - x0) * hv[c][0] + bx] = blk
    return coefs
