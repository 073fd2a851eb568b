"""Device-side resize, crop window and flip of uint8 images (fastvim_amd/resample.py, csrc/resample.hip) against the numpy
restatement of PIL's 8-bit bicubic resampler (tests/resample_ref.py, itself held to PIL and to PIL-written fixtures by
tests/test_resample_cpu.py).  Every comparison is ``torch.equal``: the device path is the host path bit for bit.

Shapes are the smallest at which the kernels can go wrong: windows of 16 x 16 and 24 x 16 (one full row band of 16 and a
partial one), 24 x 256 with a strong vertical reduction (the band is walked in sub-bands that fit the LDS tile, four-byte
stores) and 20 x 262 (two column tiles, the second 6 wide; byte stores)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import resample_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _image(rng, H, W, binary=False):
    if binary:
        return (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def _ref(samples, size):
    return torch.from_numpy(np.stack([R.resample(s["a"], crop=s.get("crop"), out_full=s.get("out_full"),
                                                 window=s.get("window", (0, 0)), size=size, flip=s.get("flip", False))
                                      for s in samples]))


def _fill(stage, samples):
    for k, s in enumerate(samples):
        stage.put(k, s["a"], crop=s.get("crop"), out_full=s.get("out_full"), window=s.get("window", (0, 0)),
                  flip=s.get("flip", False))
    stage.commit()


def _run(samples, size, capacity=1 << 20, **kw):
    from fastvim_amd.resample import ImageStage
    size = (size, size) if isinstance(size, int) else size
    stage = ImageStage(len(samples), size, capacity_bytes=capacity, **kw)
    _fill(stage, samples)
    out = torch.full((len(samples), 3) + size, 77, dtype=torch.uint8, device="cuda")
    stage.resample(out=out)
    return out.cpu(), stage


def _mismatch(got, want):
    return [(b, int((got[b] != want[b]).sum())) for b in range(got.shape[0]) if not torch.equal(got[b], want[b])]


def test_mixed_batch_of_seven():
    rng = np.random.default_rng(1)
    samples = [dict(a=_image(rng, 16, 16)),                    # identity
               dict(a=_image(rng, 5, 7)),                      # upscale
               dict(a=_image(rng, 130, 141)),                  # about 8.8x down: 37 taps
               dict(a=_image(rng, 256, 256)),                  # scale exactly 16: 65 taps
               dict(a=_image(rng, 1, 1)),
               dict(a=_image(rng, 9, 200)),                    # up on one axis, 12.5x down on the other
               dict(a=_image(rng, 37, 23, binary=True))]       # reaches the clip on both sides
    got, stage = _run(samples, 16)
    want = _ref(samples, (16, 16))
    assert stage.last_fallbacks == 0
    assert torch.equal(got, want), _mismatch(got, want)
    assert torch.equal(got[0], torch.from_numpy(samples[0]["a"].transpose(2, 0, 1).copy()))
    assert got[6].min().item() == 0 and got[6].max().item() == 255


def test_every_row_alignment_and_odd_pool_offsets():
    """Source rows of 3 w bytes with 3 w mod 4 in {0, 1, 2, 3} through the stage (16-byte-aligned starts), then the same
    sources packed back to back at odd byte offsets with a plan written by hand, through the C entry points."""
    from fastvim_amd import _lib as L
    from fastvim_amd.resample import PLAN_INTS
    rng = np.random.default_rng(2)
    samples = [dict(a=_image(rng, 11 + k, w)) for k, w in enumerate((20, 19, 22, 21))]
    assert sorted(s["a"].shape[1] * 3 % 4 for s in samples) == [0, 1, 2, 3]
    want = _ref(samples, (16, 16))
    got, _ = _run(samples, 16)
    assert torch.equal(got, want), _mismatch(got, want)
    pool, plan, off = np.zeros(4096, np.uint8), np.zeros((4, PLAN_INTS), np.int32), 1
    for k, s in enumerate(samples):
        h, w = s["a"].shape[:2]
        pool[off:off + h * w * 3] = s["a"].reshape(-1)
        plan[k, :9] = (off, 0, h, w, 16, 16, 0, 0, 0)
        off += h * w * 3 + (2, 1, 4, 0)[k]
    assert off <= 4096 and [int(v) for v in plan[:, 0]] == [1, 663, 1348, 2210]      # 1, 3, 0 and 2 mod 4
    lib = L.lib()
    d_pool, d_plan = torch.from_numpy(pool).cuda(), torch.from_numpy(plan).cuda()
    ws = torch.empty(lib.fv_resample_workspace_ints(L.i32(4), L.i32(16), L.i32(16)), dtype=torch.int32, device="cuda")
    out = torch.zeros(4, 3, 16, 16, dtype=torch.uint8, device="cuda")
    n, st = ctypes.c_longlong(4096), L.stream_of(out)
    L.check(lib.fv_resample_coeffs(L.ptr(d_plan), n, L.ptr(ws), L.i32(4), L.i32(16), L.i32(16), st), "coeffs")
    L.check(lib.fv_resample_u8(L.ptr(d_pool), n, L.ptr(d_plan), L.ptr(ws), L.ptr(out), L.i32(4), L.i32(16), L.i32(16), st), "u8")
    assert torch.equal(out.cpu(), want), _mismatch(out.cpu(), want)


def test_window_of_a_validation_resize():
    """40 x 61 source, short side to 18 (long side int(18 * 61 / 40) = 27), the centre 16 x 16: origin (1, round(5.5) = 6)."""
    from fastvim_amd.resample import ResizeCenterCrop
    rng = np.random.default_rng(3)
    a, b = _image(rng, 40, 61), _image(rng, 61, 40)
    rcc = ResizeCenterCrop(16)
    pa, pb = rcc.plan(40, 61), rcc.plan(61, 40)
    assert pa == ((18, 27), (1, 6)) and pb == ((27, 18), (6, 1))
    samples = [dict(a=a, out_full=pa[0], window=pa[1]), dict(a=b, out_full=pb[0], window=pb[1]),
               dict(a=a, out_full=(18, 27), window=(2, 11), flip=True)]
    got, _ = _run(samples, 16)
    want = _ref(samples, (16, 16))
    assert torch.equal(got, want), _mismatch(got, want)
    full = R.resize(a, 18, 27)
    assert torch.equal(got[0], torch.from_numpy(full[1:17, 6:22].transpose(2, 0, 1).copy()))


def test_flip_on_and_off_in_one_batch():
    rng = np.random.default_rng(4)
    a = _image(rng, 50, 43)
    samples = [dict(a=a, crop=(3, 5, 40, 31), flip=False), dict(a=a, crop=(3, 5, 40, 31), flip=True)]
    got, _ = _run(samples, 16)
    want = _ref(samples, (16, 16))
    assert torch.equal(got, want), _mismatch(got, want)
    assert torch.equal(got[1], got[0].flip(-1)) and not torch.equal(got[0], got[1])


def test_pil_fixtures():
    z = np.load(os.path.join(GOLDEN, "resample.npz"))
    n = len([k for k in z.files if k.startswith("in_")])
    assert n >= 12
    for k in range(n):
        a, (top, left, h, w, o_h, o_w), want = z[f"in_{k}"], (int(v) for v in z[f"meta_{k}"]), z[f"out_{k}"]
        got, stage = _run([dict(a=a, crop=(top, left, h, w)), dict(a=a, crop=(top, left, h, w), flip=True)], (o_h, o_w),
                          capacity=1 << 16)
        assert stage.last_fallbacks == 0
        assert torch.equal(got[0], torch.from_numpy(want.transpose(2, 0, 1).copy())), k
        assert torch.equal(got[1], torch.from_numpy(want[:, ::-1].transpose(2, 0, 1).copy())), k


def test_non_square_window_and_band_tail():
    """S_h = 24: a full band of 16 rows and a partial one of 8; S_w = 16."""
    rng = np.random.default_rng(5)
    samples = [dict(a=_image(rng, 24, 16)), dict(a=_image(rng, 100, 37), flip=True),
               dict(a=_image(rng, 70, 90), out_full=(29, 33), window=(5, 17)), dict(a=_image(rng, 384, 17, binary=True))]
    got, _ = _run(samples, (24, 16))
    want = _ref(samples, (24, 16))
    assert torch.equal(got, want), _mismatch(got, want)


@pytest.mark.parametrize("size", [(24, 256), (20, 262)], ids=["sub_bands_24x256", "column_tiles_20x262"])
def test_wide_windows_sub_bands_and_column_tiles(size):
    """At 256 columns the LDS tile holds 65 source rows: a band of 16 output rows reduced 8x (about 160 source rows) is
    walked in sub-bands.  262 columns are two column tiles, the second 6 wide, stored bytewise (262 is no multiple of 4)."""
    rng = np.random.default_rng(6)
    samples = [dict(a=_image(rng, 200, 300)), dict(a=_image(rng, 61, 531), flip=True), dict(a=_image(rng, 33, 47, binary=True))]
    got, _ = _run(samples, size)
    want = _ref(samples, size)
    assert torch.equal(got, want), _mismatch(got, want)


def test_out_of_range_sample_takes_the_host_fallback_or_raises():
    """300 x 20 to 16 x 16 is a reduction of 18.75: the host resizes it with PIL when PIL imports (staged as an identity
    resample, the flip still on the device), otherwise ``put`` raises; the other samples of the batch are unaffected."""
    from fastvim_amd.resample import ImageStage
    rng = np.random.default_rng(7)
    far = dict(a=_image(rng, 300, 20), flip=True)
    near = [dict(a=_image(rng, 31, 20)), dict(a=_image(rng, 256, 20), flip=True)]
    try:
        import PIL  # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False
    stage = ImageStage(3, 16, capacity_bytes=1 << 16)
    out = torch.zeros(3, 3, 16, 16, dtype=torch.uint8, device="cuda")
    stage.put(0, near[0]["a"])
    if have_pil:
        stage.put(1, far["a"], flip=True)
        samples = [near[0], far, near[1]]
    else:
        with pytest.raises(ValueError, match="sample 1 .*scale 18.75"):
            stage.put(1, far["a"], flip=True)
        stage.put(1, near[0]["a"])
        samples = [near[0], near[0], near[1]]
    stage.put(2, near[1]["a"], flip=True)
    stage.commit()
    assert stage.last_fallbacks == (1 if have_pil else 0)
    stage.resample(out=out)
    want = _ref(samples, (16, 16))
    assert torch.equal(out.cpu(), want), _mismatch(out.cpu(), want)


def test_ring_two_rounds_without_a_host_sync():
    from fastvim_amd.resample import ImageStage
    rng = np.random.default_rng(8)
    rounds = [[dict(a=_image(rng, 40 + 3 * r, 33 + k), flip=bool(k & 1)) for k in range(4)] for r in range(3)]
    stage = ImageStage(4, 16, capacity_bytes=1 << 16, slots=2)
    outs = [torch.zeros(4, 3, 16, 16, dtype=torch.uint8, device="cuda") for _ in rounds]
    for samples, out in zip(rounds, outs):      # the third round returns to the first slot
        _fill(stage, samples)
        stage.resample(out=out)
    torch.cuda.synchronize()
    for samples, out in zip(rounds, outs):
        want = _ref(samples, (16, 16))
        assert torch.equal(out.cpu(), want), _mismatch(out.cpu(), want)
    with pytest.raises(RuntimeError, match="never put"):
        stage.put(0, rounds[0][0]["a"])
        stage.commit()


def test_mae_model_fed_by_the_stage_equals_the_host_assembled_batch():
    from fastvim_amd.models_mae import MaskedAutoencoderViM
    from fastvim_amd.pixels import IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD, attach_pixel_norm
    from fastvim_amd.resample import ImageStage
    torch.manual_seed(3)
    m = MaskedAutoencoderViM(img_size=32, patch_size=8, depth=2, embed_dim=192, decoder_embed_dim=128, decoder_depth=1,
                             rms_norm=True, residual_in_fp32=True, fused_add_norm=True).cuda()
    attach_pixel_norm(m, IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD)
    rng = np.random.default_rng(9)
    samples = [dict(a=_image(rng, 75, 100), crop=(7, 11, 52, 61), flip=True), dict(a=_image(rng, 64, 48), crop=(0, 3, 40, 45))]
    x_host = _ref(samples, (32, 32)).cuda()
    noise = torch.rand(2, 16, generator=torch.Generator().manual_seed(5)).cuda()
    stage = ImageStage(2, 32, capacity_bytes=1 << 16)
    x_u8 = torch.zeros(2, 3, 32, 32, dtype=torch.uint8, device="cuda")
    _fill(stage, samples)
    stage.resample(out=x_u8)
    assert torch.equal(x_u8, x_host)
    with torch.no_grad():
        la, pa, ma = m(x_u8, mask_ratio=0.75, noise=noise)
        lb, pb, mb = m(x_host, mask_ratio=0.75, noise=noise)
    assert torch.isfinite(la).item() and torch.equal(la, lb) and torch.equal(pa, pb) and torch.equal(ma, mb)


def test_graph_replay_reads_the_plan_and_the_pool_of_the_moment():
    from fastvim_amd.resample import ImageStage
    rng = np.random.default_rng(10)
    rounds = [[dict(a=_image(rng, 20 + 9 * r + k, 50 - 7 * r), flip=bool((k + r) & 1)) for k in range(3)] for r in range(4)]
    stage = ImageStage(3, (24, 16), capacity_bytes=1 << 16, slots=1)
    x = torch.zeros(3, 3, 24, 16, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _fill(stage, rounds[0])
        stage.resample(out=x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), _ref(rounds[0], (24, 16)))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stage.resample(out=x)
    for samples in rounds[1:]:
        _fill(stage, samples)                   # a new plan and new pool contents, written between replays
        graph.replay()
        want = _ref(samples, (24, 16))
        assert torch.equal(x.cpu(), want), _mismatch(x.cpu(), want)
