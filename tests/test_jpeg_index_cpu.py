"""The JPEG index on the CPU (include/fastvim_hip.h at THE INDEX; fastvim_amd/csrc/jpeg_host.cpp builds it with the decode
core the device runs): the C++ index against the numpy restatement tests/jpeg_index_ref.py byte for byte, every group
decoded ON ITS OWN from its entry against ``jpeg.entropy_decode`` of the whole image and of sub-windows, the files that
are not indexed, and what the host refuses.  Every comparison is exact.

The files: every served fixture of tests/golden/jpeg_cases.npz without a restart interval, and the quality-100 noise files of
tests/golden/jpeg_index_cases.npz, which hold the two position cases (asserted below): a group whose first bit follows a
stuffed 0xFF 0x00 pair with bit offset 0, and a group that starts inside a byte whose predecessor in the stream is a data
0xFF (the two file bytes in front of it are 0xFF 0x00)."""
import os

import numpy as np
import pytest

import jpeg_index_ref as X
import jpeg_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEGMENTS = (1, 2, 3, 8, 1000)
_FILES = None


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


def windows(hd):
    """Three MCU windows of an image: one MCU (the last but one, or the only one), an inner rectangle, the last row."""
    mx, my = hd.mcus_x, hd.mcus_y
    one = (max(mx - 2, 0), max(my - 2, 0), 1, 1)
    inner = (1, 1, mx - 2, my - 2) if mx > 2 and my > 2 else (mx - 1, 0, 1, my)
    return one, inner, (0, my - 1, mx, 1)


def test_the_fixtures_cover_the_cases():
    names = indexable()
    assert len(names) >= 36 and {n.split("_")[1] for n in names} == {"444", "422", "420", "gray"}
    assert any("_opt_" in n for n in names) and any(n.startswith("1x1_") for n in names)


@pytest.mark.parametrize("S", SEGMENTS)
def test_index_equals_the_restatement_byte_for_byte(S):
    J = jpeg()
    for n in indexable():
        raw = files()[n]
        got, want = J.build_index(raw, S), X.build_index(raw, S)
        assert got == want, (n, S, len(got), len(want))
        info, hd = J.index_info(got), R.parse(raw)
        assert (info.nbytes, info.hash, info.height, info.width, info.subsampling) == (len(raw), X.fnv1a(raw), hd.H, hd.W, hd.cls)
        assert (info.mcus_x, info.mcus_y, info.segment_mcus, info.scan) == (hd.mcus_x, hd.mcus_y, S, hd.scan)
        assert info.groups == info.groups_per_row * hd.mcus_y == -(-hd.mcus_x // S) * hd.mcus_y
        probe = J._probe(raw)
        assert len(got) == J.L.host_lib().fv_jpeg_index_bound(probe[6], probe[7], S) == X.ENTRIES + 16 * (info.groups + 1)


@pytest.mark.parametrize("S", SEGMENTS)
def test_every_group_on_its_own_gives_the_whole_image(S):
    J = jpeg()
    for n in indexable():
        raw = files()[n]
        index = J.build_index(raw, S)
        _, want = J.entropy_decode(raw)
        got = np.concatenate([c.reshape(-1) for c in X.decode_window(raw, index)])
        assert np.array_equal(got, want), (n, S)


@pytest.mark.parametrize("S", SEGMENTS)
def test_groups_that_meet_a_window_give_the_window(S):
    J = jpeg()
    for n in indexable():
        raw = files()[n]
        index = J.build_index(raw, S)
        wins = windows(R.parse(raw))
        assert wins[0][2:] == (1, 1)
        for win in wins:
            rec, want = J.entropy_decode(raw, win)
            got = np.concatenate([c.reshape(-1) for c in X.decode_window(raw, index, win)])
            assert np.array_equal(got, want), (n, S, win)
            # the host half: the same dense record as the host decoder writes, and the staged bytes are the file's
            srec_rec, srec, pool = J.index_stage(raw, index, win, verify=True)
            assert np.array_equal(srec_rec, rec), (n, S, win)
            gx0, gw = win[0] // S, (win[0] + win[2] - 1) // S - win[0] // S + 1
            assert tuple(srec[:10]) == (1, rec[4], *win, R.parse(raw).mcus_x, S, gx0, gw)
            byte, bit, _ = X.entries_of(index)
            first = int(byte[win[1] * -(-R.parse(raw).mcus_x // S) + gx0])
            assert int(srec[23]) == first and pool[int(srec[20]):int(srec[20]) + int(srec[22])].tobytes() == raw[first:first + int(srec[22])]
            assert int(srec[22]) <= len(raw) - first and pool.size % 16 == 0


def test_both_position_cases_occur():
    """Among the groups of one MCU of the quality-100 noise files (tests/golden/gen_jpeg_index.py picks them)."""
    z = np.load(os.path.join(GOLDEN, "jpeg_index_cases.npz"))
    after_pair, inside = 0, 0
    for n in (str(n) for n in z["names"]):
        raw = files()[n]
        byte, bit, _ = X.entries_of(X.build_index(raw, 1))
        for b, k in zip(byte[:-1], bit[:-1]):
            if raw[b - 2:b] == b"\xff\x00":
                after_pair += k == 0
                inside += k > 0
    assert after_pair > 0 and inside > 0, (after_pair, inside)


def test_no_entry_rests_on_a_stuffed_zero():
    for n in indexable():
        raw = files()[n]
        byte, bit, _ = X.entries_of(X.build_index(raw, 1))
        scan = R.parse(raw).scan
        for b in byte[:-1]:
            assert not (b > scan and raw[b] == 0 and raw[b - 1] == 0xFF and _is_stuffed(raw, scan, int(b))), (n, int(b))


def _is_stuffed(raw, scan, at):
    """Whether raw[at] is a stuffed 0x00: walk the stuffed stream from the scan's first byte."""
    p = scan
    while p < at:
        p += 2 if raw[p] == 0xFF else 1
    return p != at


def test_files_that_are_not_indexed_raise_with_their_reason():
    J = jpeg()
    dri = [n for n in files() if "_rst" in n]
    assert len(dri) == 8
    for n in dri:
        with pytest.raises(ValueError, match="restart interval"):
            J.build_index(files()[n])
        with pytest.raises(X.NotIndexed, match="restart interval"):
            X.build_index(files()[n], 4)
    with pytest.raises(ValueError, match="progressive"):
        J.build_index(files()["33x47_420_progressive"])
    with pytest.raises(ValueError, match="malformed"):
        J.build_index(b"not a jpeg")
    with pytest.raises(ValueError, match="segment_mcus"):
        J.build_index(files()["33x47_420_q90_noise"], 0)
    cut = files()["33x47_420_q90_noise"]
    with pytest.raises(ValueError, match="data ends early"):
        J.build_index(cut[:len(cut) // 2])                       # the host decoder gives such a file up as well


def test_the_host_refuses_an_index_that_does_not_fit_the_file():
    J = jpeg()
    raw = files()["33x47_420_q90_noise"]
    index = J.build_index(raw, 2)
    J.index_stage(raw, index, verify=True)

    def edited(at, value, width=4):
        b = bytearray(index)
        b[at:at + width] = int(value).to_bytes(width, "little")
        return bytes(b)
    with pytest.raises(ValueError, match="not an index"):
        J.index_stage(raw, edited(0, 0x12345678))                # magic
    with pytest.raises(ValueError, match="not an index"):
        J.index_stage(raw, edited(4, 2))                         # version
    with pytest.raises(ValueError, match="another file"):
        J.index_stage(raw + b"\x00", index)                      # nbytes
    same_size = bytearray(raw)
    same_size[-3] ^= 1                                           # the same size, another file
    J.index_stage(bytes(same_size), index)                       # ... passes unverified
    with pytest.raises(ValueError, match="another file"):
        J.index_stage(bytes(same_size), index, verify=True)      # wrong hash
    with pytest.raises(ValueError, match="another file"):
        J.index_stage(raw, edited(16, 1), verify=True)           # the hash word itself
    e0 = X.ENTRIES
    with pytest.raises(ValueError, match="entry outside the scan"):
        J.index_stage(raw, edited(e0 + 16 * 3, len(raw) + 1))    # behind the file
    with pytest.raises(ValueError, match="entry outside the scan"):
        J.index_stage(raw, edited(e0 + 16 * 3, R.parse(raw).scan - 1))      # in front of the scan
    with pytest.raises(ValueError, match="entry outside the scan"):
        J.index_stage(raw, edited(e0 + 16 * 3 + 4, 8))           # bit offset 8
    byte, _, _ = X.entries_of(index)
    with pytest.raises(ValueError, match="out of order"):
        J.index_stage(raw, edited(e0 + 16 * 2, int(byte[4]) + 1))            # not monotone
    J.index_stage(raw, edited(e0 + 16 * 3, len(raw) + 1), window=(0, 0, 1, 1))     # an entry the window does not use
    with pytest.raises(ValueError, match="inconsistent header"):
        J.index_stage(raw, edited(48, 3))                        # S without its group counts
    with pytest.raises(ValueError, match="window outside"):
        J.index_stage(raw, index, window=(0, 0, 99, 1))
    with pytest.raises(ValueError):
        J.index_stage(raw, index[:-16])                          # the sentinel cut off
