"""The JPEG decode without a GPU: the numpy restatement (tests/jpeg_ref.py) against PIL-written fixtures
(tests/golden/jpeg_cases.npz, tests/golden/gen_jpeg.py) and against live PIL, and the C++ host decoder of the built library
(fastvim_amd/csrc/jpeg_host.cpp through fastvim_amd/jpeg.py) against the restatement: coefficients exactly, for whole
images and for windows; the early stop; the record; the error returns; the probe's reasons."""
import ctypes
import io
import os

import numpy as np
import pytest

import jpeg_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        z = np.load(os.path.join(GOLDEN, "jpeg_cases.npz"))
        _CASES = {str(n): (z["jpg_" + str(n)].tobytes(), z["rgb_" + str(n)]) for n in z["names"]}
    return _CASES


def served_cases():
    return {n: v for n, v in cases().items() if "progressive" not in n}


def _lib_built():
    from fastvim_amd import _lib as L
    return os.path.exists(L.LIB_PATH)


needs_lib = pytest.mark.skipif(not _lib_built(), reason="libfastvim_hip.so is not built")


# ------------------------------------------------------------------------------------------- restatement vs PIL
def test_fixture_file_covers_the_issue_list():
    names = list(cases())
    assert len(names) == 45
    for size in ("8x8", "17x23", "33x47", "64x80", "9x130", "1x1"):
        for cls in ("444", "422", "420", "gray"):
            assert any(n.startswith(f"{size}_{cls}_") for n in names), (size, cls)
    for tag in ("q20", "q75", "q100", "opt", "rstblk", "rstrow", "smooth", "noise", "edge", "progressive"):
        assert any(f"_{tag}" in n for n in names), tag
    assert os.path.getsize(os.path.join(GOLDEN, "jpeg_cases.npz")) < 1 << 20


def test_restatement_equals_fixtures():
    classes = set()
    for name, (raw, rgb) in served_cases().items():
        h, w, _, cls, ok, reason = R.probe(raw)
        assert ok and reason == R.OK and (h, w) == rgb.shape[:2], name
        assert cls == {"444": R.S444, "422": R.S422, "420": R.S420, "gray": R.GRAY}[name.split("_")[1]], name
        classes.add(cls)
        got = R.decode(raw)
        assert np.array_equal(got, rgb), (name, int((got != rgb).sum()))
    assert classes == {0, 1, 2, 3}
    assert R.probe(cases()["33x47_420_progressive"][0])[4:] == (False, R.PROGRESSIVE)


def test_restatement_crops_through_their_mcu_window():
    for name in ("33x47_420_q90_noise", "64x80_422_q90_noise", "64x80_420_q90_noise", "33x47_444_q90_noise"):
        raw, rgb = cases()[name]
        H, W = rgb.shape[:2]
        for crop in ((3, 5, 11, 13), (17, 19, 9, 7), (0, 0, 9, 9), (H - 7, W - 9, 7, 9), (1, 0, H - 1, 3), (16, 16, 16, 16)):
            t, l, h, w = crop
            assert np.array_equal(R.decode(raw, crop), rgb[t:t + h, l:l + w]), (name, crop)


def _content(kind, H, W, rng):
    if kind == "smooth":
        y, x = np.mgrid[0:H, 0:W]
        return np.stack([(y * 7 + x * 2) % 256, (x * 5 + 30) % 256, (y * 3 + x) % 256], 2).astype(np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    a = (rng.integers(0, 2, ((H + 3) // 4, (W + 3) // 4, 3)) * 255).astype(np.uint8)
    return np.kron(a, np.ones((4, 4, 1), np.uint8))[:H, :W]


def test_restatement_equals_live_pil():
    """A grid PIL encodes and decodes here: every size x content x sampling class, the save options rotating.  Every case
    is of a served class and must be decoded by the restatement: none is skipped, none goes to a fallback."""
    PIL = pytest.importorskip("PIL")
    from PIL import Image, features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this PIL is not built on libjpeg-turbo")
    rng = np.random.default_rng(5)
    options = (dict(quality=20), dict(quality=75, optimize=True), dict(quality=100), dict(quality=85, restart_marker_blocks=1),
               dict(quality=60, restart_marker_rows=1), dict(quality=95, optimize=True))
    n = 0
    for H, W in ((1, 1), (8, 8), (17, 23), (33, 47), (64, 80), (31, 16), (16, 33), (9, 130)):
        for kind in ("smooth", "noise", "edge"):
            for ss in (0, 1, 2, "gray"):
                kw = options[n % len(options)]
                im, b = Image.fromarray(_content(kind, H, W, rng)), io.BytesIO()
                if ss == "gray":
                    im.convert("L").save(b, "JPEG", **kw)
                else:
                    im.save(b, "JPEG", subsampling=ss, **kw)
                raw = b.getvalue()
                want = np.asarray(Image.open(io.BytesIO(raw)).convert("RGB"))
                assert R.probe(raw)[3:] == (3 if ss == "gray" else ss, True, R.OK), (H, W, kind, ss, kw)
                got = R.decode(raw)
                assert np.array_equal(got, want), (H, W, kind, ss, kw, int((got != want).sum()))
                n += 1
    assert n == 96


# ------------------------------------------------------------------------------------------- the C++ host decoder
def _split(rec, coef, hd):
    """The decoder's flat coefficients as the restatement's per-component arrays, by the record."""
    u = rec.view(np.uint32)
    mw, mh = int(rec[7]), int(rec[8])
    hv = [(c[1], c[2]) for c in hd.comps] if len(hd.comps) == 3 else [(1, 1)]
    out = []
    for c, (h, v) in enumerate(hv):
        off = int(u[9 + 2 * c]) | int(u[10 + 2 * c]) << 32
        out.append(coef[off:off + mw * h * mh * v * 64].reshape(mh * v, mw * h, 64))
    return out


@needs_lib
def test_host_decoder_equals_restatement_whole_images():
    from fastvim_amd import jpeg
    for name, (raw, rgb) in served_cases().items():
        hd, want, mcus = R.entropy_decode(raw)
        rec, coef = jpeg.entropy_decode(raw)
        got = _split(rec, coef, hd)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), name
        # the record, as include/fastvim_hip.h documents it
        assert list(rec[:9]) == [1, hd.H, hd.W, len(hd.comps), hd.cls, 0, 0, hd.mcus_x, hd.mcus_y], name
        assert (int(rec[15]), int(rec[16])) == (coef.size, 0) and rec[17] == coef.size // 64 and rec[18] == mcus, name
        assert not rec[19:32].any(), name
        for c, q in enumerate(R.qtables(hd)):
            assert np.array_equal(rec[32 + 64 * c:96 + 64 * c], q), name
        assert not rec[32 + 64 * len(hd.comps):].any(), name
        info = jpeg.probe(raw)
        assert info == jpeg.JpegInfo(hd.H, hd.W, hd.cls, True, "served"), name


@needs_lib
def test_host_decoder_windows_and_early_stop():
    from fastvim_amd import jpeg
    for name in ("64x80_420_q90_noise", "64x80_422_q90_noise", "64x80_444_q90_noise", "64x80_gray_q90_noise",
                 "33x47_420_rstblk_edge", "64x80_422_rstrow_smooth"):
        raw, rgb = cases()[name]
        hd = R.parse(raw)
        for win in ((0, 0, 1, 1), (1, 1, 2, 2), (hd.mcus_x - 1, hd.mcus_y - 1, 1, 1), (0, 1, hd.mcus_x, 1), (2, 0, 1, hd.mcus_y)):
            hd, want, mcus = R.entropy_decode(raw, win)
            rec, coef = jpeg.entropy_decode(raw, win)
            assert all(np.array_equal(g, w) for g, w in zip(_split(rec, coef, hd), want)), (name, win)
            assert tuple(rec[5:9]) == win and rec[18] == mcus == (win[1] + win[3] - 1) * hd.mcus_x + win[0] + win[2], (name, win)
        assert jpeg.mcu_window(hd.H, hd.W, hd.cls, (3, 5, 11, 13)) == R.mcu_window(hd.H, hd.W, hd.cls, (3, 5, 11, 13))
    # a window that ends above the bottom does not read the rest of the file: cut the file's last third off
    raw, _ = cases()["64x80_420_q90_noise"]
    cut = raw[:len(raw) * 2 // 3]
    hd, want, _ = R.entropy_decode(raw, (0, 0, 5, 1))
    rec, coef = jpeg.entropy_decode(cut, (0, 0, 5, 1))
    assert all(np.array_equal(g, w) for g, w in zip(_split(rec, coef, hd), want)) and rec[18] == 5
    with pytest.raises(ValueError):
        jpeg.entropy_decode(cut)


def _scan_start(raw):
    return R.parse(raw).scan


@needs_lib
def test_host_decoder_returns_errors():
    from fastvim_amd import _lib as L
    from fastvim_amd import jpeg

    def code(raw, capacity=None, window=None):
        info = jpeg._probe(raw)
        win = (0, 0, info[6], info[7]) if window is None else window
        n = jpeg.window_elements(info[3], win) if capacity is None else capacity
        coef, rec = np.zeros(max(n, 1), np.int16), np.zeros(jpeg.REC_INTS, np.int32)
        return L.host_lib().fv_jpeg_entropy_decode(ctypes.c_char_p(raw), ctypes.c_longlong(len(raw)), (ctypes.c_int * 4)(*win),
                                                   ctypes.c_void_p(coef.ctypes.data), ctypes.c_longlong(n),
                                                   ctypes.c_void_p(rec.ctypes.data))

    raw, _ = cases()["33x47_444_q90_noise"]
    assert code(raw) == 0
    # truncated, at every tenth of the entropy-coded data
    s = _scan_start(raw)
    for k in range(10):
        assert code(raw[:s + (len(raw) - s) * k // 10]) in (-11, -12), k
    # a corrupted Huffman stream: 128 one bits (0xFF stuffed) -- the all-ones code word is never assigned
    mid = s + (len(raw) - s) // 2
    bad = raw[:mid] + b"\xff\x00" * 16 + raw[mid + 32:]
    assert code(bad) == -12
    with pytest.raises(R.DecodeError):
        R.entropy_decode(bad)
    # a wrong restart marker
    rst, _ = cases()["33x47_444_rstblk_edge"]
    assert code(rst) == 0
    p = rst.index(b"\xff\xd1", _scan_start(rst))
    assert code(rst[:p] + b"\xff\xd4" + rst[p + 2:]) == -14
    with pytest.raises(R.DecodeError):
        R.entropy_decode(rst[:p] + b"\xff\xd4" + rst[p + 2:])
    # capacity one element short; a window outside the image
    full = jpeg.window_elements(0, (0, 0, 6, 5))
    assert code(raw, capacity=full - 1) == -15 and code(raw, capacity=0) == -15
    assert code(raw, window=(5, 0, 2, 1)) == -16 and code(raw, window=(0, 0, 0, 1)) == -16 and code(raw, window=(-1, 0, 1, 1)) == -16
    # an unserved file
    assert code(cases()["33x47_420_progressive"][0], capacity=64, window=(0, 0, 1, 1)) == -10
    # a run past 63 comes out as an error too, whatever else a random stream hits first: no mutation may pass silently wrong
    rng = np.random.default_rng(3)
    for _ in range(200):
        m = bytearray(raw)
        m[int(rng.integers(s, len(raw) - 2))] = int(rng.integers(0, 256))
        m = bytes(m)
        try:
            _, want, _ = R.entropy_decode(m)
        except R.DecodeError:
            assert code(m) != 0
        else:
            rec, coef = jpeg.entropy_decode(m)
            assert np.array_equal(np.concatenate([w.reshape(-1) for w in want]), coef)


# ------------------------------------------------------------------------------------------------------ the probe
def _segments(raw):
    """[(marker, payload)] up to and including SOS, and the rest of the file."""
    out, pos = [], 2
    while True:
        m, ln = raw[pos + 1], (raw[pos + 2] << 8) | raw[pos + 3]
        out.append((m, raw[pos + 4:pos + 2 + ln]))
        pos += 2 + ln
        if m == 0xDA:
            return out, raw[pos:]


def _join(segs, rest):
    return b"\xff\xd8" + b"".join(bytes([0xFF, m]) + (len(p) + 2).to_bytes(2, "big") + p for m, p in segs) + rest


def _edit(raw, marker, fn):
    segs, rest = _segments(raw)
    return _join([(m, fn(p) if m == marker else p) for m, p in segs], rest)


def unserved_files():
    base, _ = cases()["17x23_420_q75_noise"]
    segs, rest = _segments(base)
    out = {R.PROGRESSIVE: cases()["33x47_420_progressive"][0]}
    out[R.ARITHMETIC] = _join([(0xC9 if m == 0xC0 else m, p) for m, p in segs], rest)
    out[R.FRAME] = _join([(0xC1 if m == 0xC0 else m, p) for m, p in segs], rest)
    out[R.PRECISION] = _edit(base, 0xC0, lambda p: b"\x0c" + p[1:])
    out[R.COMPONENTS] = _edit(base, 0xC0, lambda p: p[:5] + b"\x04" + p[6:] + b"\x04\x11\x00")
    adobe = (0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x00")
    out[R.COLOUR] = _join([adobe] + [sp for sp in segs if sp[0] != 0xE0], rest)      # with a JFIF segment libjpeg reads YCbCr
    out["rgb ids"] = _join([(m, p[:6] + b"R" + p[7:9] + b"G" + p[10:12] + b"B" + p[13:] if m == 0xC0 else
                             p[:1] + b"R" + p[2:3] + b"G" + p[4:5] + b"B" + p[6:] if m == 0xDA else p)
                            for m, p in segs if m != 0xE0], rest)
    out[R.SAMPLING] = _edit(base, 0xC0, lambda p: p[:7] + b"\x12" + p[8:])
    out[R.SCANS] = _edit(base, 0xDA, lambda p: b"\x01" + p[1:3] + p[-3:])
    out[R.TABLES16] = _edit(base, 0xDB, lambda p: b"".join(bytes([0x10 | p[q]]) + b"".join(b"\x00" + p[q + 1 + k:q + 2 + k] for k in range(64))
                                                           for q in range(0, len(p), 65)))
    out[R.MALFORMED] = b"not a jpeg at all"
    return out


def test_restatement_probe_reasons():
    for want, raw in unserved_files().items():
        reason = R.COLOUR if want == "rgb ids" else want
        assert R.probe(raw)[4:] == (False, reason), want


def test_pil_agrees_the_crafted_colour_files_are_not_ycbcr():
    """The two colour cases are unserved because libjpeg reads them as RGB: PIL decodes them to other pixels than the file
    they were made from."""
    pytest.importorskip("PIL")
    from PIL import Image
    base = cases()["17x23_420_q75_noise"]
    files = unserved_files()
    for key in (R.COLOUR, "rgb ids"):
        got = np.asarray(Image.open(io.BytesIO(files[key])).convert("RGB"))
        assert got.shape == base[1].shape and not np.array_equal(got, base[1]), key


@needs_lib
def test_probe_reports_each_unserved_class():
    from fastvim_amd import jpeg
    for want, raw in unserved_files().items():
        reason = R.COLOUR if want == "rgb ids" else want
        info = jpeg.probe(raw)
        assert (info.served, info.reason, info.subsampling) == (False, jpeg.REASONS[reason], -1), want
        h, w = R.probe(raw)[:2]
        assert (info.height, info.width) == (h, w), want
        with pytest.raises(ValueError):
            jpeg.entropy_decode(raw)
    assert jpeg.REASONS == R.REASONS
    assert jpeg.probe(bytearray(cases()["8x8_444_q75_noise"][0])).served      # any bytes-like object
