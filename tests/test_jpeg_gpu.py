"""The device half of the JPEG decode (fastvim_amd/jpeg.py, csrc/jpeg.hip) against PIL-written fixtures
(tests/golden/jpeg_cases.npz) and the numpy restatement (tests/jpeg_ref.py, held to PIL by tests/test_jpeg_cpu.py).  Every
comparison is ``torch.equal``.

The images are the fixtures' (1 x 1 up to 64 x 80: one block, non-multiples of every MCU, several MCU rows and columns,
three components of different block counts in one job); the batches are large enough that both launches' grid-stride
loops cross sample borders inside a workgroup (44 samples, about 1300 blocks)."""
import os

import numpy as np
import pytest
import torch

import jpeg_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CASES = None
SENTINEL = 0xA5


def cases():
    global _CASES
    if _CASES is None:
        z = np.load(os.path.join(GOLDEN, "jpeg_cases.npz"))
        _CASES = {str(n): (z["jpg_" + str(n)].tobytes(), z["rgb_" + str(n)]) for n in z["names"]}
    return _CASES


def _stage(batch, size=16, slots=1, cls=None, **kw):
    from fastvim_amd.jpeg import JpegImageStage
    from fastvim_amd.resample import ImageStage
    if cls == "plain":
        return ImageStage(batch, size, capacity_bytes=1 << 20, slots=slots)
    return JpegImageStage(batch, size, capacity_bytes=1 << 20, coef_capacity_bytes=1 << 20, slots=slots, **kw)


def _paint(stage):
    """Sentinel bytes in the pinned and the device pixel pool of every slot: whatever the launches do not write keeps them."""
    for s in stage._slots:
        s.pool_pin.fill_(SENTINEL)
        s.pool.fill_(SENTINEL)


def _check_regions(stage, want):
    """Every sample's pool region equals ``want[i]``, and every other byte of the pool is still the sentinel."""
    s = stage._ready
    pool = s.pool.cpu().numpy()
    rest = np.ones(pool.size, bool)
    for i, w in enumerate(want):
        off, n = s.host.offset(i), w.size
        got = pool[off:off + n].reshape(w.shape)
        assert np.array_equal(got, w), (i, int((got != w).sum()))
        assert torch.equal(stage.region(i).cpu(), torch.from_numpy(np.ascontiguousarray(w))), i
        rest[off:off + n] = False
    assert (pool[rest] == SENTINEL).all(), int((pool[rest] != SENTINEL).sum())


def test_whole_images_every_fixture():
    names = [n for n in cases() if "progressive" not in n]
    assert len(names) == 44 and {n.split("_")[1] for n in names} == {"444", "422", "420", "gray"}
    assert any(n.startswith("1x1_") for n in names) and any(n.startswith("17x23_420") for n in names)
    stage = _stage(len(names))
    _paint(stage)
    for k, n in enumerate(names):
        stage.put_jpeg(k, cases()[n][0])
    stage.commit()
    stage.decode()
    assert stage.last_jpeg_fallbacks == 0 and stage.last_fallbacks == 0
    assert stage.staged_coef_bytes == sum(2 * r.size for n in names for r in R.entropy_decode(cases()[n][0])[1])
    _check_regions(stage, [cases()[n][1] for n in names])


CROPS = {  # (top, left, h, w)
    "33x47": ((3, 5, 11, 13),        # odd origin, interior: the window has real neighbours on every side
              (17, 19, 9, 7),        # odd origin just past an MCU border
              (0, 7, 9, 21),         # touches the top
              (20, 0, 9, 9),         # the left
              (24, 11, 9, 15),       # the bottom (33 is odd: the last chroma row is replicated)
              (5, 30, 13, 17),       # the right (47 is odd)
              (0, 0, 33, 47),        # the full image
              (32, 46, 1, 1)),       # the last pixel
    "64x80": ((1, 1, 30, 30), (16, 16, 16, 16), (0, 15, 17, 33), (31, 0, 2, 80), (47, 3, 17, 9), (9, 63, 21, 17), (0, 0, 64, 80),
              (15, 31, 2, 2)),
}


@pytest.mark.parametrize("cls", ["420", "422"])
def test_crops(cls):
    jobs = [(f"{size}_{cls}_q90_noise", c) for size in ("33x47", "64x80") for c in CROPS[size]]
    stage = _stage(len(jobs))
    _paint(stage)
    for k, (n, c) in enumerate(jobs):
        stage.put_jpeg(k, cases()[n][0], crop=c)
    stage.commit()
    stage.decode()
    assert stage.last_jpeg_fallbacks == 0
    want = [cases()[n][1][t:t + h, l:l + w] for n, (t, l, h, w) in jobs]
    for (n, c), w in zip(jobs, want):
        assert np.array_equal(R.decode(cases()[n][0], c), w), (n, c)           # the restatement, through the same window
    _check_regions(stage, want)


def _batches():
    """Three batches of five: per sample (fixture, crop, out_full, window, flip, staged as a file?)."""
    a = [("64x80_420_q90_noise", (5, 9, 40, 50), None, (0, 0), True, True),
         ("33x47_444_opt_noise", None, (20, 28), (2, 3), False, True),
         ("64x80_gray_rstrow_smooth", (0, 0, 64, 64), None, (0, 0), False, True),
         ("64x80_422_q90_noise", (13, 21, 33, 35), (24, 24), (4, 8), True, True),
         ("33x47_420_rstblk_edge", None, None, (0, 0), False, True)]
    b = [("17x23_420_q75_noise", None, None, (0, 0), False, True),
         ("64x80_444_q90_noise", (3, 3, 57, 71), None, (0, 0), False, False),          # put as a decoded array
         ("9x130_422_q100_edge", None, (16, 64), (0, 24), True, True),
         ("33x47_gray_q90_noise", (1, 2, 30, 40), None, (0, 0), True, False),
         ("64x80_420_rstrow_smooth", (31, 17, 33, 47), None, (0, 0), False, True)]
    c = [("1x1_420_q20_smooth", None, None, (0, 0), False, True),
         ("33x47_422_rstblk_edge", (7, 9, 21, 31), None, (0, 0), True, True),
         ("8x8_gray_q75_noise", None, None, (0, 0), False, True),
         ("64x80_444_rstrow_smooth", None, (32, 40), (16, 24), False, True),
         ("33x47_420_q90_noise", (0, 0, 33, 47), None, (0, 0), True, False)]
    for batch in (a, b, c):
        for s in batch:
            assert s[0] in cases(), s[0]
    return a, b, c


def _put_all(stage, batch, as_files):
    for k, (n, crop, out_full, window, flip, file) in enumerate(batch):
        raw, rgb = cases()[n]
        if file and as_files:
            stage.put_jpeg(k, raw, crop=crop, out_full=out_full, window=window, flip=flip)
        else:
            stage.put(k, rgb, crop=crop, out_full=out_full, window=window, flip=flip)
    stage.commit()


_WANT = None


def _want():
    """The plain ``ImageStage`` on the fixtures' RGB, once, for the three batches."""
    global _WANT
    if _WANT is None:
        plain, _WANT = _stage(5, cls="plain"), []
        for batch in _batches():
            _put_all(plain, batch, as_files=False)
            out = torch.full((5, 3, 16, 16), 77, dtype=torch.uint8, device="cuda")
            plain.resample(out=out)
            _WANT.append(out.cpu())
    return _WANT


def test_end_to_end_equals_put_of_the_decoded_image_mixed_batches_two_slot_ring():
    stage = _stage(5, slots=2)
    for batch, want in zip(_batches(), _want()):          # three batches through two slots: the first slot is used again
        _put_all(stage, batch, as_files=True)
        out = torch.full((5, 3, 16, 16), 99, dtype=torch.uint8, device="cuda")
        stage.resample(out=out)
        assert stage.last_jpeg_fallbacks == 0 and stage.last_fallbacks == 0
        assert torch.equal(out.cpu(), want), [(k, int((out.cpu()[k] != want[k]).sum())) for k in range(5)]
    assert stage.staged_coef_bytes > 0 and stage.staged_bytes > 0


def test_graph_replay_decodes_the_batch_of_the_moment():
    a, b, c = _batches()
    stage = _stage(5, slots=1)
    x = torch.zeros(5, 3, 16, 16, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _put_all(stage, a, as_files=True)
        stage.resample(out=x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), _want()[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stage.resample(out=x)
    for batch, want in ((b, _want()[1]), (c, _want()[2]), (a, _want()[0])):      # other sizes, other sampling classes
        _put_all(stage, batch, as_files=True)
        graph.replay()
        assert torch.equal(x.cpu(), want), [(k, int((x.cpu()[k] != want[k]).sum())) for k in range(5)]


def test_fallbacks_are_counted_and_identical():
    pytest.importorskip("PIL")
    import io
    from PIL import Image
    raw, rgb = cases()["33x47_420_progressive"]
    no_eoi, rgb2 = cases()["33x47_444_q90_noise"]
    no_eoi = no_eoi[:-2]                                  # the decoder needs no EOI marker: not a fallback
    rst, _ = cases()["33x47_444_rstblk_edge"]
    p = rst.index(b"\xff\xd1", R.parse(rst).scan)
    stray = rst[:p] + b"\x55" + rst[p:]                   # a stray byte in front of a restart marker: libjpeg skips it with a
    want_stray = np.asarray(Image.open(io.BytesIO(stray)).convert("RGB"))      # warning, the decoder here gives the file up
    stage = _stage(3)
    _paint(stage)
    stage.put_jpeg(0, raw, crop=(2, 3, 20, 30))
    stage.put_jpeg(1, no_eoi)
    stage.put_jpeg(2, stray, crop=(1, 1, 30, 40))
    stage.commit()
    stage.decode()
    assert stage.last_jpeg_fallbacks == 2                 # the progressive file (the probe) and the stray byte (the decoder)
    _check_regions(stage, [rgb[2:22, 3:33], rgb2, want_stray[1:31, 1:41]])
    with pytest.raises(ValueError):
        stage.put_jpeg(0, raw, crop=(0, 0, 34, 47))       # outside the image
    with pytest.raises(OSError):
        _stage(1).put_jpeg(0, b"not a jpeg")              # PIL's own exception (UnidentifiedImageError)


def test_decoded_arrays_only_equal_the_plain_stage():
    stage = _stage(5, slots=2)
    for batch, want in zip(_batches(), _want()):
        _put_all(stage, batch, as_files=False)
        out = torch.full((5, 3, 16, 16), 99, dtype=torch.uint8, device="cuda")
        stage.resample(out=out)
        assert stage.staged_coef_bytes == 0 and stage.last_jpeg_fallbacks == 0
        assert torch.equal(out.cpu(), want)
