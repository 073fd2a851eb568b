"""The packed coefficient form without a GPU (include/fastvim_hip.h, THE PACKED FORM): the host entry point
``fv_jpeg_entropy_decode_packed`` of the built library against the dense decoder it shares its MCU loop with, on the
PIL-written fixtures (tests/golden/jpeg_cases.npz).  Every comparison is exact.

The round trip goes through ``jpeg.unpack``, the numpy restatement of the format; the format's invariants are then
checked a second time on the RAW bytes, by code of this file that shares nothing with ``unpack``."""
import ctypes
import os

import numpy as np
import pytest

import jpeg_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PACKED_WORDS = (0, 9, 10, 11, 12, 13, 14, 15, 16, 25, 26, 27, 28)      # the record words the packed form may change
E_CAPACITY = -15
_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        z = np.load(os.path.join(GOLDEN, "jpeg_cases.npz"))
        _CASES = {str(n): z["jpg_" + str(n)].tobytes() for n in z["names"]}
    return _CASES


def served_cases():
    return {n: v for n, v in cases().items() if "progressive" not in n}


def _lib_built():
    from fastvim_amd import _lib as L
    return os.path.exists(L.LIB_PATH)


pytestmark = pytest.mark.skipif(not _lib_built(), reason="libfastvim_hip.so is not built")


def windows(raw):
    """None (the whole image), the top-left MCU, an interior window, the last MCU row and the last MCU column."""
    hd = R.parse(raw)
    mx, my = hd.mcus_x, hd.mcus_y
    inner = (1, 1, mx - 2, my - 2) if mx > 2 and my > 2 else (mx // 2, my // 2, 1, 1)
    return (None, (0, 0, 1, 1), inner, (0, my - 1, mx, 1), (mx - 1, 0, 1, my))


_DECODED = {}


def decoded(name, win):
    """(dense record, dense coefficients, packed record, packed bytes) of a case, decoded once and left unchanged."""
    from fastvim_amd import jpeg
    if (name, win) not in _DECODED:
        raw = cases()[name]
        _DECODED[name, win] = (*jpeg.entropy_decode(raw, win), *jpeg.entropy_decode(raw, win, packed=True))
    return _DECODED[name, win]


def all_decoded():
    for name, raw in served_cases().items():
        for win in windows(raw):
            yield (name, win), decoded(name, win)


def _i64(rec, at):
    u = rec.view(np.uint32)
    return int(u[at]) | int(u[at + 1]) << 32


def test_round_trip_every_fixture_whole_and_windows():
    from fastvim_amd import jpeg
    n = 0
    for key, (rec, coef, prec, pbytes) in all_decoded():
        assert np.array_equal(jpeg.unpack(prec, pbytes), coef), key
        same = [k for k in range(jpeg.REC_INTS) if k not in PACKED_WORDS]
        assert np.array_equal(rec[same], prec[same]), key
        blocks = int(prec[17])
        assert rec[0] == 1 and prec[0] == 2 and blocks == coef.size // 64, key
        # the plane offsets: 64 x the blocks in front of the component -- the number the dense form has in elements
        assert [_i64(prec, 9 + 2 * c) for c in range(3)] == [_i64(rec, 9 + 2 * c) for c in range(3)], key
        assert _i64(prec, 15) == pbytes.size and _i64(prec, 25) == 0 and _i64(prec, 27) == 16 * blocks, key
        n += 1
    assert n == 44 * 5


def _walk(prec, pbytes, coef, key):
    """The invariants of one case on its raw bytes; returns per block (mask, wide, dc)."""
    blocks, vbase, end = int(prec[17]), _i64(prec, 27), _i64(prec, 15)
    assert end == pbytes.size and vbase == 16 * blocks and end % 2 == 0, key
    hdr = np.frombuffer(pbytes[:vbase].tobytes(), "<u4").reshape(blocks, 4)
    dense = coef.reshape(blocks, 64).astype(np.int64)
    cur, out = vbase, []
    for b in range(blocks):
        w0, w1, w2, w3 = (int(v) for v in hdr[b])
        mask, wide, off = w0 | w1 << 32, w2 >> 31, vbase + (w2 & 0x7fffffff)
        assert mask & 1 == 0 and w3 >> 16 == 0, (key, b)
        ac = dense[b, 1:]
        assert mask == sum(1 << (int(k) + 1) for k in np.flatnonzero(ac)), (key, b)
        assert wide == int(ac.min() < -128 or ac.max() > 127), (key, b)
        assert off % 2 == 0 and off == cur, (key, b)             # in block order, each interval begins where the last ended
        nbytes = bin(mask).count("1") * (1 + wide)
        cur = off + nbytes
        if nbytes % 2:
            assert pbytes[cur] == 0, (key, b)                    # the pad byte
            cur += 1
        out.append((mask, wide, np.int16(np.uint16(w3))))
    assert cur == end, key                                       # intervals and pad bytes tile [value base, bytes written)
    return out


def test_format_invariants_on_the_raw_bytes_and_class_coverage():
    from fastvim_amd import jpeg
    zero = dc_only = wide = full = total = 0
    for key, (rec, coef, prec, pbytes) in all_decoded():
        blocks = _walk(prec, pbytes, coef, key)
        assert pbytes.size <= jpeg.packed_bound(len(blocks)), key
        if key[1] is None:                                       # whole images: every block of the fixtures once
            total += len(blocks)
            zero += sum(m == 0 and dc == 0 for m, _, dc in blocks)
            dc_only += sum(m == 0 and dc != 0 for m, _, dc in blocks)
            wide += sum(w for _, w, _ in blocks)
            full += sum(m == (1 << 64) - 2 for m, _, _ in blocks)
    assert total == 3110
    assert zero >= 1 and dc_only >= 1 and wide >= 1 and full >= 1, (zero, dc_only, wide, full)
    assert jpeg.packed_bound(1) == 142 and jpeg.packed_bound(3110) == 3110 * 142 and jpeg.packed_bound(0) == 0


def _call(raw, win, capacity, guard=64, fill=0xA5):
    """The packed entry point on a 16-byte aligned buffer of ``capacity`` bytes with ``guard`` painted bytes behind it:
    (return code, record, the buffer, the guard)."""
    from fastvim_amd import _lib as L
    from fastvim_amd import jpeg
    buf = jpeg._aligned_bytes(capacity + guard)
    buf[:] = fill
    rec = np.zeros(jpeg.REC_INTS, np.int32)
    rc = L.host_lib().fv_jpeg_entropy_decode_packed(ctypes.c_char_p(raw), ctypes.c_longlong(len(raw)), (ctypes.c_int * 4)(*win),
                                                    ctypes.c_void_p(buf.ctypes.data), ctypes.c_longlong(capacity),
                                                    ctypes.c_void_p(rec.ctypes.data))
    return rc, rec, buf[:capacity], buf[capacity:]


@pytest.mark.parametrize("name", ["33x47_420_q90_noise", "64x80_422_q90_noise", "33x47_444_q90_noise", "64x80_gray_q90_noise"])
def test_capacity_exact_succeeds_one_byte_less_is_refused(name):
    raw = cases()[name]
    _, _, prec, pbytes = decoded(name, None)
    win = tuple(int(v) for v in prec[5:9])
    assert pbytes.size > 16 * int(prec[17])                      # the case has values
    rc, rec, buf, guard = _call(raw, win, pbytes.size)
    assert rc == 0 and np.array_equal(rec, prec) and np.array_equal(buf, pbytes) and (guard == 0xA5).all()
    rc, _, _, guard = _call(raw, win, pbytes.size - 1)
    assert rc == E_CAPACITY and (guard == 0xA5).all()
    for cap in (0, 16 * int(prec[17]) - 1, 16 * int(prec[17]), (16 * int(prec[17]) + pbytes.size) // 2):
        rc, _, buf, guard = _call(raw, win, cap)
        assert rc == E_CAPACITY and (guard == 0xA5).all(), cap


def _codes(raw):
    """(dense code, packed code) for the whole image the header states, each with room for all of it."""
    from fastvim_amd import _lib as L
    from fastvim_amd import jpeg
    info = jpeg._probe(raw)
    win = (0, 0, max(info[6], 1), max(info[7], 1))
    n = jpeg.window_elements(info[3], win) if info[4] else 64
    coef, rec = np.zeros(n, np.int16), np.zeros(jpeg.REC_INTS, np.int32)
    dense = L.host_lib().fv_jpeg_entropy_decode(ctypes.c_char_p(raw), ctypes.c_longlong(len(raw)), (ctypes.c_int * 4)(*win),
                                                ctypes.c_void_p(coef.ctypes.data), ctypes.c_longlong(n),
                                                ctypes.c_void_p(rec.ctypes.data))
    return dense, _call(raw, win, jpeg.packed_bound(n // 64))[0]


def test_error_codes_equal_the_dense_decoder():
    raw = cases()["17x23_420_q75_noise"]
    seen = set()
    for n in range(len(raw) + 1):
        dense, packed = _codes(raw[:n])
        assert dense == packed, n
        seen.add(dense)
    assert {0, -10, -11} <= seen, seen                           # complete, cut inside the headers, cut inside the scan
    assert _codes(cases()["33x47_420_progressive"]) == (-10, -10)
    # a window outside the image, and an output that is not 16-byte aligned
    assert _call(raw, (0, 0, 3, 1), 1 << 12)[0] == -16
    from fastvim_amd import _lib as L
    from fastvim_amd import jpeg
    buf, rec = jpeg._aligned_bytes(4096), np.zeros(jpeg.REC_INTS, np.int32)
    rc = L.host_lib().fv_jpeg_entropy_decode_packed(ctypes.c_char_p(raw), ctypes.c_longlong(len(raw)), (ctypes.c_int * 4)(0, 0, 1, 1),
                                                    ctypes.c_void_p(buf.ctypes.data + 8), ctypes.c_longlong(2048),
                                                    ctypes.c_void_p(rec.ctypes.data))
    assert rc == -1                                              # FV_ERR_INVALID


def test_unpack_refuses_bytes_that_are_too_short():
    from fastvim_amd import jpeg
    _, coef, prec, pbytes = decoded("33x47_420_q90_noise", None)
    assert np.array_equal(jpeg.unpack(prec, pbytes), coef)
    with pytest.raises(ValueError):
        jpeg.unpack(prec, pbytes[:-2])
    with pytest.raises(ValueError):
        jpeg.unpack(prec, pbytes[:16 * int(prec[17]) - 1])
    # a sample moved inside a pool: the caller's offsets
    moved = prec.copy()
    moved[25], moved[27] = 48, 48 + 16 * int(prec[17])
    assert np.array_equal(jpeg.unpack(moved, np.concatenate([np.full(48, 0xEE, np.uint8), pbytes])), coef)
