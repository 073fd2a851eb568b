"""The packed coefficient form on the device (``JpegImageStage(..., coef_format="packed")``, ``fv_jpeg_idct_packed`` of
csrc/jpeg.hip) against the dense form of the same stage and against the PIL-written pixels of the fixtures
(tests/golden/jpeg_cases.npz).  Every comparison is ``torch.equal`` / ``np.array_equal``.

The shapes are the fixtures' own, 1 x 1 to 64 x 80 pixels, in batches of 8: what can go wrong is per block (the mask, the
value offset, int8 against int16 values, DC only) and per 8-lane group, not per size; tests/test_jpeg_packed_cpu.py asserts
that the fixtures hold every block class.  Each stage has small pools of its own."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CASES = None
SENTINEL = 0xA5
B = 8


def cases():
    global _CASES
    if _CASES is None:
        z = np.load(os.path.join(GOLDEN, "jpeg_cases.npz"))
        _CASES = {str(n): (z["jpg_" + str(n)].tobytes(), z["rgb_" + str(n)]) for n in z["names"]}
    return _CASES


def _stage(fmt, slots=1, size=16, **kw):
    from fastvim_amd.jpeg import JpegImageStage
    kw.setdefault("coef_capacity_bytes", 1 << 18 if fmt == "dense" else 1 << 17)
    return JpegImageStage(B, size, capacity_bytes=1 << 18, slots=slots, coef_format=fmt, **kw)


def _paint(stage):
    for s in stage._slots:
        s.pool_pin.fill_(SENTINEL)
        s.pool.fill_(SENTINEL)


def _regions(stage):
    return [stage.region(i).cpu() for i in range(B)]


def _decode_jobs(stage, jobs):
    """``jobs``: 8 x (fixture, crop); the pool regions after ``decode()``."""
    for k, (n, c) in enumerate(jobs):
        stage.put_jpeg(k, cases()[n][0], crop=c)
    stage.commit()
    stage.decode()
    assert stage.last_jpeg_fallbacks == 0 and stage.last_fallbacks == 0
    return _regions(stage)


def _check_jobs(jobs):
    packed, dense = _stage("packed"), _stage("dense")
    for lo in range(0, len(jobs), B):
        part = jobs[lo:lo + B]
        _paint(packed)
        got, ref = _decode_jobs(packed, part), _decode_jobs(dense, part)
        used = np.zeros(packed.capacity, bool)
        for k, (n, c) in enumerate(part):
            rgb = cases()[n][1]
            t, l, h, w = (0, 0, *rgb.shape[:2]) if c is None else c
            assert torch.equal(got[k], ref[k]), (n, c, int((got[k] != ref[k]).sum()))
            assert np.array_equal(got[k].numpy(), rgb[t:t + h, l:l + w]), (n, c)
            off = packed._ready.host.offset(k)
            used[off:off + h * w * 3] = True
        # what the launches did not have to write keeps the sentinel
        pool = packed._ready.pool.cpu().numpy()
        assert (pool[~used] == SENTINEL).all(), int((pool[~used] != SENTINEL).sum())
        # the packed pool is the smaller one (what the form is for), and the stage reports its used part
        assert 0 < packed.staged_coef_bytes < dense.staged_coef_bytes
        assert packed.staged_coef_bytes == packed._ready.jused and packed.staged_coef_bytes % 16 == 0


def test_whole_images_every_fixture():
    names = [n for n in cases() if "progressive" not in n]
    assert len(names) == 44 and {n.split("_")[1] for n in names} == {"444", "422", "420", "gray"}
    names += names[:4]                                    # six full batches of 8
    _check_jobs([(n, None) for n in names])


CROPS = {  # (top, left, h, w): the crops of tests/test_jpeg_gpu.py -- they start and end inside an MCU
    "33x47": ((3, 5, 11, 13), (17, 19, 9, 7), (0, 7, 9, 21), (20, 0, 9, 9), (24, 11, 9, 15), (5, 30, 13, 17), (0, 0, 33, 47),
              (32, 46, 1, 1)),
    "64x80": ((1, 1, 30, 30), (16, 16, 16, 16), (0, 15, 17, 33), (31, 0, 2, 80), (47, 3, 17, 9), (9, 63, 21, 17), (0, 0, 64, 80),
              (15, 31, 2, 2)),
}


@pytest.mark.parametrize("cls", ["420", "422"])
def test_crops(cls):
    _check_jobs([(f"{size}_{cls}_q90_noise", c) for size in ("33x47", "64x80") for c in CROPS[size]])


def _batches():
    """Three batches of eight: per sample (fixture, crop, out_full, window, flip, staged as a file?).  The progressive
    fixture is a fallback of ``put_jpeg``; the sizes of the batches' packed pools differ."""
    a = [("64x80_420_q90_noise", (5, 9, 40, 50), None, (0, 0), True, True),
         ("33x47_444_opt_noise", None, (20, 28), (2, 3), False, True),
         ("64x80_gray_rstrow_smooth", (0, 0, 64, 64), None, (0, 0), False, True),
         ("64x80_422_q90_noise", (13, 21, 33, 35), (24, 24), (4, 8), True, True),
         ("33x47_420_rstblk_edge", None, None, (0, 0), False, True),
         ("33x47_420_progressive", (2, 3, 20, 30), None, (0, 0), False, True),
         ("64x80_444_q90_noise", (3, 3, 57, 71), None, (0, 0), False, False),          # put as a decoded array
         ("17x23_420_q75_noise", None, None, (0, 0), True, True)]
    b = [("17x23_420_q75_noise", None, None, (0, 0), False, True),
         ("33x47_gray_q90_noise", (1, 2, 30, 40), None, (0, 0), True, False),
         ("9x130_422_q100_edge", None, (16, 64), (0, 24), True, True),
         ("1x1_420_q20_smooth", None, None, (0, 0), False, True),
         ("64x80_420_rstrow_smooth", (31, 17, 33, 47), None, (0, 0), False, True),
         ("8x8_gray_q75_noise", None, None, (0, 0), False, True),
         ("33x47_420_progressive", None, None, (0, 0), True, True),
         ("33x47_422_rstblk_edge", (7, 9, 21, 31), None, (0, 0), True, True)]
    c = [("64x80_444_rstrow_smooth", None, (32, 40), (16, 24), False, True),
         ("33x47_420_q90_noise", (0, 0, 33, 47), None, (0, 0), True, False),
         ("64x80_444_q90_noise", None, None, (0, 0), False, True),
         ("64x80_420_q90_noise", None, None, (0, 0), False, True),
         ("64x80_422_q90_noise", None, None, (0, 0), True, True),
         ("33x47_444_q90_noise", (3, 5, 11, 13), None, (0, 0), False, True),
         ("64x80_gray_q90_noise", None, None, (0, 0), False, True),
         ("33x47_420_progressive", (1, 1, 30, 40), None, (0, 0), False, True)]
    for batch in (a, b, c):
        assert len(batch) == B and all(s[0] in cases() for s in batch)
    return a, b, c


def _put_all(stage, batch, order=None, threads=0):
    def one(k):
        n, crop, out_full, window, flip, file = batch[k]
        raw, rgb = cases()[n]
        if file:
            stage.put_jpeg(k, raw, crop=crop, out_full=out_full, window=window, flip=flip)
        else:
            stage.put(k, rgb, crop=crop, out_full=out_full, window=window, flip=flip)
    order = range(len(batch)) if order is None else order
    if threads:
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(one, order))
    else:
        for k in order:
            one(k)
    stage.commit()


_WANT = None


def _want():
    """The DENSE stage, eager, on the three batches: computed once, shared, left unchanged."""
    global _WANT
    if _WANT is None:
        pytest.importorskip("PIL")                        # the progressive fixture is PIL's to decode
        dense, _WANT = _stage("dense"), []
        for batch in _batches():
            _put_all(dense, batch)
            out = torch.full((B, 3, 16, 16), 77, dtype=torch.uint8, device="cuda")
            dense.resample(out=out)
            assert dense.last_jpeg_fallbacks == sum(s[0].endswith("progressive") and s[5] for s in batch) == 1
            _WANT.append(out.cpu())
    return _WANT


def test_mixed_batches_with_a_fallback_two_slot_ring():
    want = _want()
    stage = _stage("packed", slots=2)
    for batch, w in zip(_batches(), want):                # three batches through two slots: the first slot is used again
        _put_all(stage, batch)
        out = torch.full((B, 3, 16, 16), 99, dtype=torch.uint8, device="cuda")
        stage.resample(out=out)
        assert stage.last_jpeg_fallbacks == 1 and stage.last_fallbacks == 0
        assert torch.equal(out.cpu(), w), [(k, int((out.cpu()[k] != w[k]).sum())) for k in range(B)]
    assert stage.staged_coef_bytes > 0 and stage.staged_bytes > 0


def test_graph_replay_decodes_the_batch_of_the_moment():
    want = _want()
    a, b, c = _batches()
    stage = _stage("packed", slots=1)
    x = torch.zeros(B, 3, 16, 16, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _put_all(stage, a)
        stage.resample(out=x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), want[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stage.resample(out=x)
    sizes = []
    for batch, w in ((b, want[1]), (c, want[2]), (a, want[0])):
        _put_all(stage, batch)
        sizes.append(stage.staged_coef_bytes)
        graph.replay()
        assert torch.equal(x.cpu(), w), [(k, int((x.cpu()[k] != w[k]).sum())) for k in range(B)]
    assert len(set(sizes)) == 3, sizes                    # the packed sizes of the replayed batches differ


def test_put_order_changes_the_layout_not_the_pixels():
    want = _want()[2]
    batch = _batches()[2]
    layouts = []
    for order, threads in ((range(B), 0), ((5, 2, 7, 0, 3, 6, 1, 4), 0), (range(B - 1, -1, -1), 4)):
        stage = _stage("packed")
        _put_all(stage, batch, order=order, threads=threads)
        out = torch.full((B, 3, 16, 16), 99, dtype=torch.uint8, device="cuda")
        stage.resample(out=out)
        assert torch.equal(out.cpu(), want), (tuple(order), threads)
        r = stage._ready.records
        layouts.append(tuple(int(r[k, 25]) for k in range(B) if r[k, 0] == 2))
        assert len(layouts[-1]) == 6 and len(set(layouts[-1])) == 6
    assert layouts[0] != layouts[1]                       # the same samples lie elsewhere in the pool


def test_capacity_overflow_raises_before_anything_is_launched():
    from fastvim_amd import jpeg
    raw = cases()["64x80_420_q90_noise"][0]
    rec, pbytes = jpeg.entropy_decode(raw, packed=True)
    blocks = int(rec[17])
    # the packed pool: room for one such sample and not for two
    stage = _stage("packed", coef_capacity_bytes=pbytes.size + 64, plane_capacity_bytes=1 << 16)
    stage.put_jpeg(0, raw)
    with pytest.raises(ValueError, match=rf"sample 1 \({pbytes.size} packed coefficient bytes.*coef_capacity_bytes = {stage.coef_bytes}"):
        stage.put_jpeg(1, raw)
    # the plane workspace: 64 bytes per block
    stage2 = _stage("packed", plane_capacity_bytes=64 * blocks + 64)
    stage2.put_jpeg(0, raw)
    with pytest.raises(ValueError, match=rf"sample 3 \({64 * blocks} plane bytes.*plane_capacity_bytes = {stage2.plane_bytes}"):
        stage2.put_jpeg(3, raw)
    for s in (stage, stage2):
        assert s._ready is None                           # nothing was committed, so nothing can have been launched
        with pytest.raises(RuntimeError):
            s.decode()
        assert not any(s._slots[0].host.filled[1:])       # and the refused sample took no place
    # the default plane capacity is four times the packed pool; the dense form has no such keyword
    assert _stage("packed").plane_bytes == 4 * (1 << 17)
    with pytest.raises(ValueError):
        _stage("dense", plane_capacity_bytes=1 << 16)
    with pytest.raises(ValueError):
        _stage("zigzag")
