"""Host side of the device geometry (fastvim_amd/resample.py) and its numpy reference (tests/resample_ref.py): the reference
against PIL itself and against the committed PIL fixtures, the validation plan, timm's random-resized-crop draw, the range
predicate of the library against its Python restatement, and the packing of the plan and the pool."""
import math
import os
import random

import numpy as np
import pytest
import torch

import resample_ref as R
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _image(rng, H, W, binary):
    if binary:
        return (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def fixtures():
    z = np.load(os.path.join(GOLDEN, "resample.npz"))
    n = len([k for k in z.files if k.startswith("in_")])
    return [(z[f"in_{k}"], tuple(int(v) for v in z[f"meta_{k}"]), z[f"out_{k}"]) for k in range(n)]


# ------------------------------------------------------------------------------------------------- the reference itself
def test_reference_equals_pil_byte_for_byte():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    # (H, W, o_h, o_w): scale exactly 1, exactly 16, just above 16 (66 and 67 taps wanted: 65 after the clamp at the ends)
    fixed = [(24, 31, 24, 31), (64, 80, 4, 5), (65, 81, 4, 5), (90, 33, 5, 2), (1, 1, 1, 1), (1, 90, 40, 1), (90, 1, 1, 40)]
    cases = [(H, W, oh, ow) for H, W, oh, ow in fixed]
    while len(cases) < 240:
        cases.append((int(rng.integers(1, 91)), int(rng.integers(1, 91)), int(rng.integers(1, 41)), int(rng.integers(1, 41))))
    bad = []
    for n, (H, W, oh, ow) in enumerate(cases):
        a = _image(rng, H, W, binary=n % 3 == 0)
        if n % 2:                              # a crop rectangle: taps clamp at ITS edge
            h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
            i, j = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        else:
            i, j, h, w = 0, 0, H, W
        want = np.asarray(Image.fromarray(a).crop((j, i, j + w, i + h)).resize((ow, oh), Image.BICUBIC))
        got = R.resize(a[i:i + h, j:j + w], oh, ow)
        if not np.array_equal(want, got):
            bad.append(((H, W, oh, ow), (i, j, h, w), int((want != got).sum())))
    assert not bad, bad


def test_reference_window_and_flip_are_slices_of_the_full_resize():
    rng = np.random.default_rng(8)
    a = _image(rng, 40, 61, False)
    full = R.resize(a, 18, 27)
    got = R.resample(a, out_full=(18, 27), window=(1, 6), size=(16, 16))
    assert np.array_equal(got, full[1:17, 6:22].transpose(2, 0, 1))
    got = R.resample(a, out_full=(18, 27), window=(1, 6), size=(16, 16), flip=True)
    assert np.array_equal(got, full[1:17, 6:22][:, ::-1].transpose(2, 0, 1))
    got = R.resample(a, crop=(3, 4, 20, 30), size=(16, 24))
    assert np.array_equal(got, R.resize(a[3:23, 4:34], 16, 24).transpose(2, 0, 1))


def test_reference_equals_the_pil_fixtures():
    fx = fixtures()
    assert len(fx) >= 12
    for a, (top, left, h, w, o_h, o_w), want in fx:
        assert want.shape == (o_h, o_w, 3) and 8 <= o_h <= 32 and 8 <= o_w <= 32
        assert np.array_equal(R.resize(a[top:top + h, left:left + w], o_h, o_w), want)


def test_fixtures_are_what_pil_writes():
    Image = pytest.importorskip("PIL.Image")
    for a, (top, left, h, w, o_h, o_w), want in fixtures():
        got = np.asarray(Image.fromarray(a).crop((left, top, left + w, top + h)).resize((o_w, o_h), Image.BICUBIC))
        assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------- validation plan
@pytest.mark.parametrize("img_size", [16, 24])
def test_resize_center_crop_plan_equals_pil_resize_and_centre_crop(img_size):
    Image = pytest.importorskip("PIL.Image")
    from fastvim_amd.resample import ResizeCenterCrop
    rcc = ResizeCenterCrop(img_size)
    size = int(img_size / 0.875)
    assert rcc.size == size
    rng = np.random.default_rng(9)
    for H, W in [(40, 61), (61, 40), (33, 33), (19, 57), (100, 23), (size, size + 7)]:
        a = _image(rng, H, W, False)
        # torchvision's Resize(size) and CenterCrop(img_size), restated
        if W <= H:
            ow, oh = size, int(size * H / W)
        else:
            oh, ow = size, int(size * W / H)
        top, left = int(round((oh - img_size) / 2.0)), int(round((ow - img_size) / 2.0))
        want = np.asarray(Image.fromarray(a).resize((ow, oh), Image.BICUBIC))[top:top + img_size, left:left + img_size]
        out_full, window = rcc.plan(H, W)
        assert out_full == (oh, ow) and window == (top, left)
        got = R.resample(a, out_full=out_full, window=window, size=(img_size, img_size))
        assert np.array_equal(got, want.transpose(2, 0, 1))


def test_resize_center_crop_ratio_is_one_above_224():
    from fastvim_amd.resample import ResizeCenterCrop
    assert ResizeCenterCrop(224).size == 256 and ResizeCenterCrop(224).plan(500, 375) == ((341, 256), (58, 16))
    r = ResizeCenterCrop(384)
    assert r.crop_ratio == 1.0 and r.size == 384 and r.plan(500, 375) == ((512, 384), (64, 0))


# ----------------------------------------------------------------------------------------------- random resized crop
def _timm_box(H, W, scale, ratio):
    """The issue's listing (timm's RandomResizedCropAndInterpolation.get_params), transcribed."""
    for _ in range(10):
        target_area = random.uniform(*scale) * H * W
        aspect = math.exp(random.uniform(math.log(ratio[0]), math.log(ratio[1])))
        w = int(round(math.sqrt(target_area * aspect)))
        h = int(round(math.sqrt(target_area / aspect)))
        if w <= W and h <= H:
            i = random.randint(0, H - h)
            j = random.randint(0, W - w)
            return i, j, h, w
    in_ratio = W / H
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        w = W
        h = H
    return (H - h) // 2, (W - w) // 2, h, w


SIZES = [(375, 500), (500, 333), (200, 200), (64, 600), (10, 400), (400, 10), (8, 8), (224, 224)]


@pytest.mark.parametrize("scale", [(0.08, 1.0), (0.2, 1.0)])
def test_random_resized_crop_draw_is_timms_stream(scale):
    from fastvim_amd.resample import RandomResizedCrop
    rrc = RandomResizedCrop(224, scale=scale, hflip=0.0)
    for seed in (0, 1, 2):
        random.seed(seed)
        got = [rrc.draw(H, W) for H, W in SIZES * 4]
        state = random.getstate()
        random.seed(seed)
        want = [_timm_box(H, W, scale, (3. / 4., 4. / 3.)) for H, W in SIZES * 4]
        assert [g[:4] for g in got] == want and random.getstate() == state
        assert all(g[4] is False for g in got)
        for (i, j, h, w, _), (H, W) in zip(got, SIZES * 4):
            assert 0 <= i and 0 <= j and 1 <= h and 1 <= w and i + h <= H and j + w <= W


def test_random_resized_crop_central_fallback():
    from fastvim_amd.resample import RandomResizedCrop
    rrc = RandomResizedCrop(224, hflip=0.0)
    random.seed(5)
    before = random.getstate()
    assert rrc.draw(10, 400) == (0, (400 - 13) // 2, 10, 13, False)        # h = H, w = round(10 * 4 / 3)
    random.setstate(before)
    for _ in range(10):                        # exactly ten failed attempts were drawn: two uniforms each, no randint
        random.uniform(0.08, 1.0)
        random.uniform(math.log(3. / 4.), math.log(4. / 3.))
    after = random.getstate()
    random.setstate(before)
    rrc.draw(10, 400)
    assert random.getstate() == after
    assert rrc.draw(400, 10) == ((400 - 13) // 2, 0, 13, 10, False)        # w = W, h = round(10 / (3 / 4))


def test_random_resized_crop_flip_draw():
    from fastvim_amd.resample import RandomResizedCrop
    state = torch.get_rng_state()
    random.seed(0)
    RandomResizedCrop(224, hflip=0.0).draw(375, 500)
    assert torch.equal(torch.get_rng_state(), state)                       # hflip == 0: torch's generator is not touched
    torch.manual_seed(11)
    want = [bool(torch.rand(1) < 0.5) for _ in range(16)]
    torch.manual_seed(11)
    rrc = RandomResizedCrop(224)
    assert [rrc.draw(300, 300)[4] for _ in range(16)] == want and True in want and False in want
    g = torch.Generator().manual_seed(3)
    want = [bool(torch.rand(1, generator=g) < 0.5) for _ in range(8)]
    state = torch.get_rng_state()
    rrc = RandomResizedCrop(224, generator=torch.Generator().manual_seed(3))
    assert [rrc.draw(300, 300)[4] for _ in range(8)] == want
    assert torch.equal(torch.get_rng_state(), state)


# ------------------------------------------------------------------------------------------ predicate, plan and pool
def _built():
    from fastvim_amd import _lib
    return os.path.exists(_lib.LIB_PATH)


def test_predicate_agrees_with_the_python_range_check():
    from fastvim_amd import resample as RS
    assert _built(), "the library is not built"
    grid = []
    for batch in (0, 1, 4096, 4097):
        grid.append((batch, 16, 16, 16, 16, 16, 16, 0, 0))
    for s in (7, 8, 224, 1024, 1025):
        grid.append((2, s, 16, 40, 40, max(s, 16), 16, 0, 0))
        grid.append((2, 16, s, 40, 40, 16, max(s, 16), 0, 0))
    for src in (0, 1, 255, 256, 257, 16384, 16385):
        for o in (16, 17, 1024, 1025, 65536, 65537):
            grid.append((2, 16, 16, src, 40, o, 16, 0, 0))
            grid.append((2, 16, 16, 40, src, 16, o, 0, 0))
    for o, win in ((18, 0), (18, 2), (18, 3), (18, -1), (16, 0), (16, 1), (15, 0)):
        grid.append((2, 16, 16, 40, 40, o, 27, win, 0))
        grid.append((2, 16, 16, 40, 40, 27, o, 0, win))
    yes = 0
    for g in grid:
        assert RS.resample_ok(*g) == RS.served(*g), g
        yes += RS.served(*g)
    assert 0 < yes < len(grid)
    assert RS.served(2, 16, 16, 256, 256, 16, 16, 0, 0) and not RS.served(2, 16, 16, 257, 256, 16, 16, 0, 0)
    from fastvim_amd import _lib
    n = _lib.lib().fv_resample_workspace_ints(_lib.i32(3), _lib.i32(24), _lib.i32(16))
    assert n == RS.workspace_ints(3, 24, 16) == 3 * 40 * 67


def test_host_plan_packing_alignment_and_overflow():
    from fastvim_amd.resample import ALIGN, PLAN_INTS, HostPlan
    assert _built(), "the library is not built"
    rng = np.random.default_rng(3)
    hp = HostPlan(4, (24, 16), capacity_bytes=4096)
    imgs = [_image(rng, 5, 7, False), _image(rng, 9, 11, False), _image(rng, 30, 40, False), _image(rng, 3, 3, False)]
    hp.put(0, imgs[0], flip=True)
    hp.put(2, imgs[2], crop=(3, 5, 20, 21), out_full=(30, 20), window=(3, 2))
    hp.put(1, imgs[1])
    offs = [hp.offset(i) for i in range(3)]
    assert offs == [0, 1376, 112] and all(o % ALIGN == 0 for o in offs)     # 5*7*3 = 105 -> 112; 112 + 20*21*3 = 1372 -> 1376
    assert hp.plan.shape == (4, PLAN_INTS) and hp.plan.dtype == np.int32
    assert hp.plan[0].tolist() == [0, 0, 5, 7, 24, 16, 0, 0, 1, 0, 0, 0]
    assert hp.plan[2].tolist() == [112, 0, 20, 21, 30, 20, 3, 2, 0, 0, 0, 0]
    assert np.array_equal(hp.pool[112:112 + 1260].reshape(20, 21, 3), imgs[2][3:23, 5:26])
    assert np.array_equal(hp.pool[1376:1376 + 297].reshape(9, 11, 3), imgs[1])
    with pytest.raises(RuntimeError, match="never put"):
        hp.check_complete()
    with pytest.raises(ValueError, match="already put"):
        hp.put(1, imgs[1])
    with pytest.raises(ValueError, match="window"):
        hp.put(3, imgs[3], out_full=(24, 17), window=(0, 2))
    with pytest.raises(ValueError, match="crop"):
        hp.put(3, imgs[3], crop=(0, 0, 4, 3))
    with pytest.raises(ValueError, match="uint8"):
        hp.put(3, imgs[3].astype(np.float32))
    hp.put(3, imgs[3])
    hp.check_complete()
    assert hp.fallbacks == 0
    small = HostPlan(2, 16, capacity_bytes=16 + 16 * 16 * 3)
    small.put(0, _image(rng, 2, 2, False))
    with pytest.raises(ValueError, match="overflows capacity_bytes"):
        small.put(1, _image(rng, 16, 17, False))
    small.put(1, _image(rng, 16, 16, False))                                # exactly to the end
    # a 64-bit offset survives the two plan words
    big = HostPlan(1, 16, capacity_bytes=64)
    big.plan.view(np.uint32)[0, :2] = ((5 << 32 | 0x90000010) & 0xffffffff, 5)
    assert big.offset(0) == 5 << 32 | 0x90000010


def test_host_plan_fallback_beyond_the_range():
    pytest.importorskip("PIL")
    from fastvim_amd.resample import HostPlan
    assert _built(), "the library is not built"
    rng = np.random.default_rng(4)
    a = _image(rng, 300, 20, False)                                          # scale 18.75 down
    hp = HostPlan(1, 16, capacity_bytes=1024)
    hp.put(0, a, flip=True)
    assert hp.fallbacks == 1 and hp.plan[0].tolist() == [0, 0, 16, 16, 16, 16, 0, 0, 1, 0, 0, 0]
    assert np.array_equal(hp.pool[:768].reshape(16, 16, 3), R.resize(a, 16, 16))
