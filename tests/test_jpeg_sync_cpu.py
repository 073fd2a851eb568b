"""Index entries made without an index, on the CPU (include/fastvim_hip.h at ENTRIES MADE ON THE DEVICE):
``fv_jpeg_sync_stage`` stages a file without decoding a Huffman code and ``fv_jpeg_sync_host`` runs the passes and rounds of
``fv_jpeg_sync`` serially over the core the device compiles (fastvim_amd/csrc/jpeg_sync_core.h).  The oracle is the project's
own serial builder: the 16 bytes of every entry written must equal those ``jpeg.build_index`` holds for the same group.
Every comparison is exact.

The files: every indexable fixture of tests/golden/jpeg_cases.npz and jpeg_index_cases.npz.  The compared set is asserted to
hold all four sampling classes, the index's two position cases, a subsequence boundary on a stuffed 0x00, a sample that
needed more than two rounds, a sample of exactly one subsequence and a block that straddles a boundary."""
import os
import re

import numpy as np
import pytest

import jpeg_index_ref as X
import jpeg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SEGMENTS, SUBSEQS = (1, 3, 1000), (16, 64, 128)
_FILES, _SEEN = None, {}


def files():
    global _FILES
    if _FILES is None:
        _FILES = {}
        for npz in ("jpeg_cases.npz", "jpeg_index_cases.npz"):
            z = np.load(os.path.join(GOLDEN, npz))
            _FILES.update({str(n): z["jpg_" + str(n)].tobytes() for n in z["names"]})
    return _FILES


def indexable():
    return [n for n in files() if "_rst" not in n and "progressive" not in n]


def jpeg():
    import fastvim_amd.build as fb
    fb.build()
    from fastvim_amd import jpeg
    return jpeg


def windows(mx, my):
    return [(0, 0, mx, my)] + ([(1, 1, mx - 2, my - 2)] if mx > 2 and my > 2 else [])


def entries_of_window(J, raw, S, win, mx):
    """The serial builder's entries of the groups the window meets: (rows, group columns, 16) uint8."""
    ent = np.frombuffer(J.build_index(raw, S), np.uint8)[J.INDEX_HEAD_BYTES:].reshape(-1, 16)
    gpr, gx0 = -(-mx // S), win[0] // S
    gw = (win[0] + win[2] - 1) // S - gx0 + 1
    return np.stack([ent[(win[1] + y) * gpr + gx0:(win[1] + y) * gpr + gx0 + gw] for y in range(win[3])])


def made(job, pool, rows):
    return pool[int(job[17]):int(job[17]) + 16 * int(job[9]) * rows].reshape(rows, int(job[9]), 16)


@pytest.mark.parametrize("L", SUBSEQS)
@pytest.mark.parametrize("S", SEGMENTS)
def test_entries_equal_the_serial_builders(S, L):
    J = jpeg()
    seen = _SEEN.setdefault((S, L), {"classes": set(), "rounds": 0, "one": 0, "stuffed": 0})
    for n in indexable():
        raw = files()[n]
        info = J._probe(raw)
        mx, my = info[6], info[7]
        for win in windows(mx, my):
            rec, srec, job, pool = J.sync_stage(raw, win, S, L)
            assert job[24] == 0, (n, S, L, win, int(job[24]))
            assert np.array_equal(made(job, pool, win[3]), entries_of_window(J, raw, S, win, mx)), (n, S, L, win)
            # the dense record is the host decoder's, the stream record the index stage's but for the staged range
            want_rec, _ = J.entropy_decode(raw, win)
            assert np.array_equal(rec, want_rec), (n, S, L, win)
            hd = R.parse(raw)
            assert tuple(srec[:10]) == (1, info[3], *win, mx, S, win[0] // S, int(job[9]))
            assert int(srec[23]) == hd.scan and int(srec[18]) == int(job[17]) and int(srec[20]) == int(job[10]) and int(srec[22]) == int(job[12])
            scan = pool[int(job[10]):int(job[10]) + int(job[12])].tobytes()
            assert scan == raw[hd.scan:hd.scan + len(scan)] and raw[hd.scan + len(scan)] == 0xFF and raw[hd.scan + len(scan) + 1] != 0
            assert int(job[16]) == -(-len(scan) // L) and pool.size % 16 == 0
            seen["classes"].add(n.split("_")[1])
            seen["rounds"] = max(seen["rounds"], int(job[25]))
            seen["one"] += int(job[16]) == 1
            seen["stuffed"] += sum(scan[p] == 0 and scan[p - 1] == 0xFF for p in range(L, len(scan), L))


def test_the_compared_set_holds_the_required_cases():
    J = jpeg()
    for S in SEGMENTS:                                       # whatever ran before, the cases are counted over the whole set
        for L in SUBSEQS:
            if (S, L) not in _SEEN:
                test_entries_equal_the_serial_builders(S, L)
    assert all(s["classes"] == {"444", "422", "420", "gray"} for s in _SEEN.values())
    assert max(s["rounds"] for s in _SEEN.values()) > 2                         # a sample that needed more than two rounds
    assert sum(s["one"] for s in _SEEN.values()) > 0                            # a sample of exactly one subsequence
    assert sum(s["stuffed"] for s in _SEEN.values()) > 0                        # a boundary on a stuffed 0x00
    # the index's position cases among the compared entries (S = 1, whole image): A: the first bit follows a stuffed pair
    # with bit offset 0, B: it lies inside a byte whose predecessor in the stream is a data 0xFF
    after_pair = inside = straddle = 0
    for n in indexable():
        raw = files()[n]
        byte, bit, _ = X.entries_of(J.build_index(raw, 1))
        for b, k in zip(byte[:-1], bit[:-1]):
            if raw[b - 2:b] == b"\xff\x00":
                after_pair += k == 0
                inside += k > 0
        if "_gray_" in n:
            # one block per MCU: a block straddles boundary p unless a block starts exactly at (p, bit 0)
            scan, starts = R.parse(raw).scan, {(int(b), int(k)) for b, k in zip(byte, bit)}
            for L in SUBSEQS:
                straddle += sum((scan + p, 0) not in starts for p in range(L, int(byte[-1]) - scan, L))
    assert after_pair > 0 and inside > 0 and straddle > 0, (after_pair, inside, straddle)


def test_refusals():
    J = jpeg()
    dri = [n for n in files() if "_rst" in n]
    assert len(dri) == 8
    for n in dri:
        with pytest.raises(ValueError) as e:
            J.sync_stage(files()[n])
        assert e.value.args[1:] == (-10, 11)                                     # FV_JPEG_E_UNSERVED, FV_JPEG_R_RESTART
        with pytest.raises(ValueError, match="restart interval"):
            J.build_index(files()[n])                                            # the builder's code for the same file
    with pytest.raises(ValueError) as e:
        J.sync_stage(files()["33x47_420_progressive"])
    assert e.value.args[1:] == (-10, 1)                                          # FV_JPEG_R_PROGRESSIVE
    with pytest.raises(ValueError) as e:
        J.sync_stage(b"not a jpeg")
    assert e.value.args[1:] == (-10, 9)
    raw = files()["64x80_444_q90_noise"]
    scan_bytes = int(J.sync_stage(raw, run=False)[2][12])
    with pytest.raises(ValueError) as e:
        J.sync_stage(raw, max_scan_bytes=scan_bytes - 1)
    assert e.value.args[1] == -20                                                # FV_JPEG_E_SCAN_SIZE
    J.sync_stage(raw, max_scan_bytes=scan_bytes)
    # capacity: one byte less than what the stage takes is refused without a write (sync_stage asserts the pool untouched)
    used = J.sync_stage(raw, run=False)[3].size
    with pytest.raises(ValueError) as e:
        J.sync_stage(raw, pool_capacity_bytes=used - 1)
    assert e.value.args[1] == -15
    assert J.sync_stage(raw, pool_capacity_bytes=used)[2][24] == 0
    for L in (0, 8, 24, 2048):
        with pytest.raises(ValueError) as e:
            J.sync_stage(raw, subseq_bytes=L)
        assert e.value.args[1] == -1                                             # FV_ERR_INVALID
    with pytest.raises(ValueError) as e:
        J.sync_stage(raw, window=(0, 0, 99, 1))
    assert e.value.args[1] == -16


def test_fill_bytes_inside_the_scan_are_refused():
    J = jpeg()
    raw = files()["64x80_444_q90_noise"]
    scan = R.parse(raw).scan
    at = raw.index(b"\xff\x00", scan + 40)
    filled = raw[:at] + b"\xff" + raw[at:]                                       # 0xFF 0xFF 0x00: libjpeg skips the fill byte
    with pytest.raises(ValueError, match="data ends early"):
        J.build_index(filled)
    with pytest.raises(ValueError) as e:
        J.sync_stage(filled)
    assert e.value.args[1] == -11                                                # the builder's code


def test_a_job_that_does_not_fit_is_skipped_with_a_status():
    import ctypes
    J = jpeg()
    raw = files()["33x47_420_q90_noise"]
    rec, srec, job, pool = J.sync_stage(raw, run=False)
    lib = J.L.host_lib()
    scratch = np.zeros(8 * (int(job[16]) + 1), np.uint32)
    for word, value in ((12, int(job[12]) + (1 << 20)), (16, int(job[16]) + 1), (15, 48), (17, pool.size), (21, 2), (9, 99)):
        j, p = job.copy(), pool.copy()
        j[word] = value
        rc = lib.fv_jpeg_sync_host(ctypes.c_void_p(p.ctypes.data), ctypes.c_longlong(p.size), ctypes.c_void_p(j.ctypes.data),
                                   ctypes.c_void_p(scratch.ctypes.data), ctypes.c_longlong(int(job[16]) + 1))
        assert rc == 0 and j[24] == 5 and np.array_equal(p, pool), (word, int(j[24]))


def test_corrupt_streams_terminate_with_a_status_or_the_serial_entries():
    J = jpeg()
    rng = np.random.default_rng(7)
    gave_up = agreed = 0
    for n in ("64x80_420_q90_noise", "33x47_444_opt_noise", "64x80_gray_q75_noise", "64x80_422_q100_noise_s96"):
        raw = files()[n]
        info, hd = J._probe(raw), R.parse(raw)
        mx, my = info[6], info[7]
        win = (0, 0, mx, my)
        byte0 = X.entries_of(J.build_index(raw, 1))[0]
        end = int(byte0[-1])
        # a scan cut short: the whole image needs MCUs that are gone
        intact = entries_of_window(J, raw, 1, win, mx)
        for cut in (hd.scan + (end - hd.scan) // 2, hd.scan + 5, end - 1):
            _, _, job, pool = J.sync_stage(raw[:cut], win, 1, 64)
            if job[24] != 0:
                assert job[24] == 6 and (made(job, pool, my) == 0xFF).all(), (n, cut, int(job[24]))      # and no entry written
                gave_up += 1
            else:                                                                # only the last MCU's tail is gone
                assert np.array_equal(made(job, pool, my), intact), (n, cut)
        assert J.sync_stage(raw[:hd.scan + (end - hd.scan) // 2], win, 1, 64)[2][24] == 6
        # one flipped byte
        for _ in range(40):
            at = int(rng.integers(hd.scan, end))
            mutated = bytearray(raw)
            mutated[at] ^= 1 << int(rng.integers(0, 8))
            mutated = bytes(mutated)
            L = (16, 64, 128)[int(rng.integers(0, 3))]
            try:
                _, _, job, pool = J.sync_stage(mutated, win, 1, L)
            except ValueError as e:
                assert e.args[1] in (-11, -20)                                   # the flip made a marker or a fill byte
                continue
            if job[24] != 0:
                gave_up += 1
                continue
            got = made(job, pool, my)
            try:
                want = entries_of_window(J, mutated, 1, win, mx)                 # the serial decoder gets through: the same entries
                assert np.array_equal(got, want), (n, at, L)
                agreed += 1
            except ValueError:
                # it gives up somewhere behind the last group start: the entries in front of the damage are the file's own
                intact = entries_of_window(J, raw, 1, win, mx)
                before = intact[..., :4].copy().view("<u4")[..., 0] < at
                assert np.array_equal(got[before], intact[before]), (n, at, L)
    assert gave_up > 0 and agreed > 0, (gave_up, agreed)


def test_new_symbols_are_declared_and_the_abi_version_stays():
    import ctypes
    from fastvim_amd import _lib
    jpeg()
    text = open(os.path.join(ROOT, "include", "fastvim_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(fv_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("fv_jpeg_sync_stage", "fv_jpeg_sync_host", "fv_jpeg_sync_table_ints", "fv_jpeg_sync"):
        assert s in declared and s in _lib.C_ABI_SYMBOLS and hasattr(lib, s), s
    assert "ENTRIES MADE ON THE DEVICE" in text and "fv_jpeg_sync were ADDED" in text
    assert int(re.search(r"#define\s+FV_ABI_VERSION\s+(\d+)", hdr).group(1)) == 3 == lib.fv_version()
    lib.fv_jpeg_sync_table_ints.restype = ctypes.c_longlong
    assert lib.fv_jpeg_sync_table_ints(8) == 8 * 32 and lib.fv_jpeg_sync_table_ints(0) == 0
    assert os.path.exists(os.path.join(ROOT, "fastvim_amd", "csrc", "jpeg_sync.hip"))
    assert os.path.exists(os.path.join(ROOT, "fastvim_amd", "csrc", "jpeg_sync_core.h"))
