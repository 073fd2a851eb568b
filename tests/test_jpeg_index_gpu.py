"""The indexed JPEG path on the device (fastvim_amd/jpeg.py ``put_jpeg_indexed``, csrc/jpeg.hip ``fv_jpeg_huff``): the
coefficients a lane per group writes against the host decoder's, the pixels against PIL's, the resampled batch against
the ``put_jpeg`` stage's, mixed batches, a replayed graph, and the dense path left as it was.  Every comparison is exact.

Fixtures are at most 64 x 80 and a batch is 8 samples: all four sampling classes, optimised Huffman tables, the
quality-100 noise files with the index's position cases, whole images and crops (a crop of one MCU row, a crop whose
window starts inside a group, a crop narrower than a group)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CASES, _INDEX = None, {}
SENTINEL = 0x5A5A


def cases():
    global _CASES
    if _CASES is None:
        _CASES = {}
        for npz in ("jpeg_cases.npz", "jpeg_index_cases.npz"):
            z = np.load(os.path.join(GOLDEN, npz))
            _CASES.update({str(n): (z["jpg_" + str(n)].tobytes(), z["rgb_" + str(n)]) for n in z["names"]})
    return _CASES


def noise100():
    return sorted(n for n in cases() if "_q100_noise_s" in n)


def index(name, S):
    from fastvim_amd import jpeg
    if (name, S) not in _INDEX:
        _INDEX[(name, S)] = jpeg.build_index(cases()[name][0], S)
    return _INDEX[(name, S)]


def _stage(batch=8, slots=1, stream=1 << 19, **kw):
    from fastvim_amd.jpeg import JpegImageStage
    return JpegImageStage(batch, 16, capacity_bytes=1 << 20, coef_capacity_bytes=1 << 20, slots=slots, stream_capacity_bytes=stream, **kw)


def batch_a():
    """(fixture, crop, out_full, window, flip)"""
    q = noise100()
    return [("64x80_444_q90_noise", None, None, (0, 0), False),
            ("64x80_422_q90_noise", (13, 21, 33, 35), (24, 24), (4, 8), True),
            ("64x80_420_q90_noise", (5, 9, 40, 50), None, (0, 0), True),
            ("64x80_gray_q90_noise", (31, 0, 2, 80), None, (0, 0), False),          # one MCU row... two: rows 3 and 4
            ("33x47_420_opt_noise", None, (20, 28), (2, 3), False),
            ("33x47_444_opt_noise", (3, 5, 11, 13), None, (0, 0), False),
            (q[0], (15, 31, 2, 2), None, (0, 0), True),                             # a window of very few MCUs
            (q[-1], None, None, (0, 0), False)]


def batch_b():
    q = noise100()
    return [("33x47_gray_opt_noise", None, None, (0, 0), True),
            ("33x47_422_opt_noise", (17, 19, 9, 7), None, (0, 0), False),
            (q[-1], (9, 63, 21, 17), None, (0, 0), False),
            ("64x80_420_q90_noise", None, (32, 40), (16, 24), False),
            ("17x23_420_q75_noise", None, None, (0, 0), False),
            ("8x8_gray_q75_noise", None, None, (0, 0), False),
            ("64x80_444_q90_noise", (47, 3, 17, 9), None, (0, 0), True),
            ("1x1_420_q20_smooth", None, None, (0, 0), False)]


def _put(stage, batch, S, how="indexed"):
    """``how``: "indexed", "jpeg", or a per-sample list of "indexed" / "jpeg" / "array"."""
    for k, (n, crop, out_full, window, flip) in enumerate(batch):
        raw, rgb = cases()[n]
        h = how if isinstance(how, str) else how[k]
        if h == "indexed":
            stage.put_jpeg_indexed(k, raw, index(n, S), crop=crop, out_full=out_full, window=window, flip=flip, verify=(k % 2 == 0))
        elif h == "jpeg":
            stage.put_jpeg(k, raw, crop=crop, out_full=out_full, window=window, flip=flip)
        else:
            stage.put(k, rgb, crop=crop, out_full=out_full, window=window, flip=flip)
    stage.commit()


_WANT = {}


def want(which):
    """The resampled batch of the ``put_jpeg`` stage (the parent's code path), once per batch."""
    if which not in _WANT:
        from fastvim_amd.jpeg import JpegImageStage
        st = JpegImageStage(8, 16, capacity_bytes=1 << 20, coef_capacity_bytes=1 << 20, slots=1)
        _put(st, {"a": batch_a, "b": batch_b}[which](), 0, how="jpeg")
        out = torch.full((8, 3, 16, 16), 77, dtype=torch.uint8, device="cuda")
        st.resample(out=out)
        assert st.last_jpeg_fallbacks == 0
        _WANT[which] = out.cpu()
    return _WANT[which]


@pytest.mark.parametrize("S", [1, 3, 1000])
@pytest.mark.parametrize("which", ["a", "b"])
def test_coefficients_pixels_status(S, which):
    from fastvim_amd import jpeg
    batch = {"a": batch_a, "b": batch_b}[which]()
    assert {n.split("_")[1] for n, *_ in batch_a() + batch_b()} == {"444", "422", "420", "gray"}
    assert any("_opt_" in n for n, *_ in batch) and any("_q100_" in n for n, *_ in batch)
    stage = _stage()
    for s in stage._slots:
        s.coef.fill_(SENTINEL)                             # every coefficient of a window is WRITTEN, zeros included
        s.pool.fill_(0xA5)
    _put(stage, batch, S)
    assert stage.staged_coef_bytes == 0 and stage.staged_stream_bytes > 0      # no coefficient crossed the link
    stage.decode()
    torch.cuda.synchronize()
    assert stage.last_jpeg_fallbacks == 0 and stage.last_fallbacks == 0
    assert torch.equal(stage.stream_status(), torch.zeros(8, dtype=torch.int32))
    s = stage._ready
    coef = s.coef.cpu().numpy()
    rest = np.ones(coef.size, bool)
    top = coef.size
    for k, (n, crop, *_) in enumerate(batch):
        raw, rgb = cases()[n]
        info = jpeg.probe(raw)
        win = jpeg.mcu_window(info.height, info.width, info.subsampling, crop)
        rec, ref = jpeg.entropy_decode(raw, win)
        got_rec = s.records[k]
        base = jpeg._rec_i64(got_rec, 9)
        assert base + ref.size == top, (k, base, ref.size, top)          # reserved from the top downward, nothing between
        top = base
        assert np.array_equal(coef[base:base + ref.size], ref), (n, S, int((coef[base:base + ref.size] != ref).sum()))
        rest[base:base + ref.size] = False
        # the record is the host decoder's, but for the offsets (moved by the base) and the caller's words
        moved = got_rec.copy()
        for c in range(3):
            if jpeg._rec_i64(rec, 9 + 2 * c) or c == 0:
                jpeg._rec_add(moved, 9 + 2 * c, -base)
        moved[19:25] = 0
        assert np.array_equal(moved, rec), (n, S)
        t, l, h, w = (0, 0, info.height, info.width) if crop is None else crop
        assert torch.equal(stage.region(k).cpu(), torch.from_numpy(np.ascontiguousarray(rgb[t:t + h, l:l + w]))), (n, S)
    assert (coef[rest] == SENTINEL).all(), int((coef[rest] != SENTINEL).sum())


@pytest.mark.parametrize("S", [1, 3, 1000])
def test_resample_equals_the_put_jpeg_stage(S):
    for which, batch in (("a", batch_a()), ("b", batch_b())):
        stage = _stage(slots=2)
        _put(stage, batch, S)
        out = torch.full((8, 3, 16, 16), 99, dtype=torch.uint8, device="cuda")
        stage.resample(out=out)
        assert stage.last_jpeg_fallbacks == 0 and stage.staged_coef_bytes == 0
        assert torch.equal(out.cpu(), want(which)), [(k, int((out.cpu()[k] != want(which)[k]).sum())) for k in range(8)]
        assert torch.equal(stage.stream_status(), torch.zeros(8, dtype=torch.int32))


def test_mixed_batch_of_arrays_files_and_indexed_files():
    from fastvim_amd import jpeg
    how = ["indexed", "jpeg", "array", "indexed", "jpeg", "indexed", "array", "indexed"]
    stage = _stage(slots=2)
    _put(stage, batch_a(), 3, how=how)
    out = torch.full((8, 3, 16, 16), 99, dtype=torch.uint8, device="cuda")
    stage.resample(out=out)
    assert stage.last_jpeg_fallbacks == 0
    assert torch.equal(out.cpu(), want("a"))
    host = 0
    for k, (n, crop, *_) in enumerate(batch_a()):
        if how[k] == "jpeg":
            info = jpeg.probe(cases()[n][0])
            host += 2 * jpeg.window_elements(info.subsampling, jpeg.mcu_window(info.height, info.width, info.subsampling, crop))
    assert stage.staged_coef_bytes == host > 0             # only the files decoded on the host sent coefficients
    assert torch.equal(stage.stream_status(), torch.zeros(8, dtype=torch.int32))


def test_graph_replay_decodes_the_batch_of_the_moment():
    stage = _stage(slots=1)
    x = torch.zeros(8, 3, 16, 16, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _put(stage, batch_a(), 3)
        stage.resample(out=x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), want("a"))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stage.resample(out=x)
    # other files, other windows, another S, at the same pool addresses: stale coefficients would show
    for which, batch, S in (("b", batch_b(), 1), ("a", batch_a(), 1000), ("b", batch_b(), 3)):
        _put(stage, batch, S)
        graph.replay()
        assert torch.equal(x.cpu(), want(which)), (which, S, [(k, int((x.cpu()[k] != want(which)[k]).sum())) for k in range(8)])
    assert torch.equal(stage.stream_status(), torch.zeros(8, dtype=torch.int32))


def test_the_dense_path_is_unchanged_without_a_stream_pool():
    from fastvim_amd import _lib as L
    from fastvim_amd.jpeg import JpegImageStage
    stage = JpegImageStage(8, 16, capacity_bytes=1 << 20, coef_capacity_bytes=1 << 20, slots=1)
    assert stage.stream_bytes == 0 and not hasattr(stage._slots[0], "stream") and not hasattr(stage._slots[0], "stable")
    lib, launches = L.lib(), []
    real = {name: getattr(lib, name) for name in ("fv_jpeg_huff", "fv_jpeg_idct", "fv_jpeg_idct_packed", "fv_jpeg_rgb")}
    try:
        for name, fn in real.items():
            lib._wrapped[name] = lambda *a, _n=name, _f=fn: (launches.append(_n), _f(*a))[1]
        _put(stage, batch_a(), 0, how="jpeg")
        stage.decode()
    finally:
        lib._wrapped.update(real)
    assert launches == ["fv_jpeg_idct", "fv_jpeg_rgb"]
    for k, (n, crop, *_) in enumerate(batch_a()):
        rgb = cases()[n][1]
        t, l, h, w = (0, 0, *rgb.shape[:2]) if crop is None else crop
        assert torch.equal(stage.region(k).cpu(), torch.from_numpy(np.ascontiguousarray(rgb[t:t + h, l:l + w]))), n
    with pytest.raises(RuntimeError, match="stream_capacity_bytes"):
        stage.put_jpeg_indexed(0, cases()["8x8_gray_q75_noise"][0], index("8x8_gray_q75_noise", 1))
    with pytest.raises(RuntimeError):
        stage.stream_status()


def test_arguments_and_refusals():
    from fastvim_amd.jpeg import JpegImageStage
    with pytest.raises(ValueError, match="packed"):
        JpegImageStage(8, 16, capacity_bytes=1 << 20, coef_capacity_bytes=1 << 20, coef_format="packed", stream_capacity_bytes=1 << 16)
    raw, idx = cases()["64x80_420_q90_noise"][0], index("64x80_420_q90_noise", 3)
    other = cases()["64x80_422_q90_noise"][0]
    stage = _stage(batch=8)
    with pytest.raises(ValueError, match="bytes, not"):
        stage.put_jpeg_indexed(0, other, idx)                              # the index of another file
    with pytest.raises(ValueError, match="not an index"):
        stage.put_jpeg_indexed(0, raw, b"\0" * len(idx))
    flipped = bytearray(raw)
    flipped[-5] ^= 4
    with pytest.raises(ValueError, match="another file"):
        stage.put_jpeg_indexed(0, bytes(flipped), idx, verify=True)
    with pytest.raises(ValueError, match="does not lie inside"):
        stage.put_jpeg_indexed(0, raw, idx, crop=(0, 0, 65, 80))
    small = _stage(batch=8, stream=4096)
    with pytest.raises(ValueError, match="stream_capacity_bytes"):
        small.put_jpeg_indexed(0, raw, idx)
    tight = _stage(batch=8, segment_capacity=3)
    with pytest.raises(ValueError, match="segment_capacity"):
        tight.put_jpeg_indexed(0, raw, idx)
    # a refusal leaves the sample free: the same slot is then put for real, and the batch decodes
    for k in range(8):
        stage.put_jpeg_indexed(k, raw, idx, crop=(8 * k, 0, 8, 80))
    stage.commit()
    stage.decode()
    rgb = cases()["64x80_420_q90_noise"][1]
    for k in range(8):
        assert torch.equal(stage.region(k).cpu(), torch.from_numpy(np.ascontiguousarray(rgb[8 * k:8 * k + 8])))
    assert torch.equal(stage.stream_status(), torch.zeros(8, dtype=torch.int32))
