"""Device-side RandAugment (fastvim_amd/randaug.py, csrc/randaug.hip) against the numpy restatement of PIL's operations
(tests/randaug_ref.py, itself held to PIL and to PIL-written fixtures by tests/test_randaug_cpu.py) and against the
fixtures directly.  Every comparison is ``torch.equal``: the device path is the host path byte for byte.

Shapes are the smallest at which the kernels can go wrong: 8x8 (one row tile; equalize's ``step == 0``), 24x40 and 40x24
(three and five row tiles of 8; rotation centre and translate fractions of non-square images), 37x41 (a row tile of 5;
planes of 1517 bytes start at every alignment, so the byte heads and tails of the dword stores are all used) and one
224x224 batch of 4."""
import os
import random

import numpy as np
import pytest
import torch

import randaug_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MEAN = (0.485, 0.456, 0.406)
RECIPE = "rand-m9-mstd0.5-inc1"


def _ra(size, batch, config=RECIPE):
    from fastvim_amd.randaug import RandAugment
    return RandAugment(config, size, MEAN, batch)


def _image(rng, H, W, kind=0):
    """0 random, 1 smooth, 2 few-valued, 3 constant"""
    kind %= 4
    if kind == 0:
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == 1:
        s = rng.integers(0, 256, (H + 4, W + 4, 3)).astype(np.float64)
        for _ in range(2):
            s = (s + np.roll(s, 1, 0) + np.roll(s, -1, 0) + np.roll(s, 1, 1) + np.roll(s, -1, 1)) / 5
        return s[2:-2, 2:-2].round().astype(np.uint8)
    if kind == 2:
        return (rng.integers(0, 3, (H, W, 3)) * 100 + 20).astype(np.uint8)
    return np.broadcast_to(rng.integers(0, 256, 3).astype(np.uint8), (H, W, 3)).copy()


def _planar(images):
    return torch.from_numpy(np.ascontiguousarray(np.stack([a.transpose(2, 0, 1) for a in images])))


def _run(ra, images):
    """commit + apply on the batch; checks that ``src`` is left unchanged"""
    src = _planar(images).cuda()
    keep = src.clone()
    out = torch.full_like(src, 77)
    ra.commit()
    assert ra.apply(src, out) is out
    assert torch.equal(src, keep)
    return out.cpu()


def _want(ra, images):
    return _planar([R.apply_plan(a, ra.records[k]) for k, a in enumerate(images)])


def _mismatch(ra, got, want):
    return [(b, [r.kind for r in ra.records[b]], int((got[b] != want[b]).sum())) for b in range(got.shape[0])
            if not torch.equal(got[b], want[b])]


def _forced_args(ra, seed):
    """every op of both lists with an argument drawn as the recipe draws it"""
    from fastvim_amd.randaug import OPS, OPS_INCREASING
    random.seed(seed)
    names = list(OPS) + [n for n in OPS_INCREASING if n not in OPS]
    return [(n, ra.level_args(n, max(0., min(random.gauss(9, 0.5), 10.)))) for n in names]


@pytest.mark.parametrize("position", [0, 1, 2])
@pytest.mark.parametrize("size", [(24, 40), (37, 41)], ids=["24x40", "37x41"])
def test_every_op_in_every_layer_position(size, position):
    """Three layers; sample k runs op k of both lists (21 names) at layer ``position`` and two other ops of the
    list in the other layers, so neighbouring samples run different kinds in every launch and both intermediate buffers
    are used."""
    ra = _ra(size, 21, "rand-m9-n3-mstd0.5-inc1")
    ops = _forced_args(ra, 7 + position)
    assert len(ops) == 21
    rng = np.random.default_rng(20 + position)
    images = [_image(rng, *size, kind=k) for k in range(21)]
    for k in range(21):
        for layer in range(3):
            name, args = ops[k] if layer == position else ops[(k + 4 + 3 * layer) % 21]
            ra.put(k, layer, ra.record(name, *args))
    assert {ra.records[k][position].kind for k in range(21)} == set(range(1, 12))
    got, want = _run(ra, images), _want(ra, images)
    assert torch.equal(got, want), _mismatch(ra, got, want)


@pytest.mark.parametrize("size", [(8, 8), (24, 40), (40, 24), (37, 41)], ids=["8x8", "24x40", "40x24", "37x41"])
def test_drawn_plans_with_skipped_ops(size):
    """The recipe's own draws (half of the layers are skipped) on 24 images of all four types; samples 0..3 are forced to
    the histogram ops on a random and on a constant image (8x8: equalize's step is 0; constant: one bin, hi <= lo)."""
    ra = _ra(size, 24)
    np.random.seed(31)
    random.seed(32)
    drawn = [ra.draw(k) for k in range(24)]
    assert any(n is None for layers in drawn for n, _ in layers) and any(n is not None for layers in drawn for n, _ in layers)
    for k, name in enumerate(("Equalize", "AutoContrast", "Equalize", "AutoContrast")):
        ra.put(k, 0, ra.record(name))
    rng = np.random.default_rng(33)
    images = [_image(rng, *size, kind=(0, 0, 3, 3)[k] if k < 4 else k) for k in range(24)]
    if size == (8, 8):
        h = R.histogram(images[0])
        assert all((int(c.sum()) - int(c[np.nonzero(c)[0][-1]])) // 255 == 0 for c in h)
    got, want = _run(ra, images), _want(ra, images)
    assert torch.equal(got, want), _mismatch(ra, got, want)


def test_batch_of_four_at_224():
    """Equalize on an image whose table exceeds 255 before the clip, then a rotation; the recipe's other families."""
    ra = _ra(224, 4)
    rng = np.random.default_rng(40)
    images = [R.equalize_overflow_image(), _image(rng, 224, 224, 1), _image(rng, 224, 224, 0), _image(rng, 224, 224, 1)]
    plans = [(("Equalize", ()), ("Rotate", (-26.7,))), (("SharpnessIncreasing", (1.83,)), ("ContrastIncreasing", (0.21,))),
             (("AutoContrast", ()), ("ColorIncreasing", (1.77,))), (("ShearY", (0.28,)), ("TranslateXRel", (-0.41,)))]
    for k, layers in enumerate(plans):
        for layer, (name, args) in enumerate(layers):
            ra.put(k, layer, ra.record(name, *args))
    got, want = _run(ra, images), _want(ra, images)
    assert torch.equal(got, want), _mismatch(ra, got, want)
    eq = R.apply_record(images[0], ra.records[0][0])
    assert (eq == 255).sum() > (images[0] == 255).sum()          # the clipped entries map to 255, not to 0


def test_blend_factors_below_above_and_exactly_one():
    ra = _ra((37, 41), 24, "rand-n1")
    rng = np.random.default_rng(50)
    images = []
    for k in range(24):
        name, factor = ("Color", "Contrast", "Brightness", "Sharpness")[k % 4], (0.0, 0.1, 0.55, 1.0, 1.9, 3.5)[k // 4]
        ra.put(k, 0, ra.record(name, factor))
        images.append(_image(rng, 37, 41, kind=k // 4 + k % 4))
    got, want = _run(ra, images), _want(ra, images)
    assert torch.equal(got, want), _mismatch(ra, got, want)
    for k in range(12, 16):                                        # factor exactly 1: the image
        assert torch.equal(got[k], _planar(images[k:k + 1])[0])
    assert torch.equal(got[2], torch.zeros_like(got[2]))           # brightness 0: the degenerate, black


def test_constant_images_and_fixed_tables_at_their_ends():
    """One bin (autocontrast ``hi <= lo``, equalize ``len(histo) <= 1``), two bins, posterize to 0 bits, solarize at 0 and
    256, solarize-add 0 and 128."""
    ra = _ra((24, 40), 12, "rand-n1")
    rng = np.random.default_rng(60)
    const = _image(rng, 24, 40, 3)
    two = const.copy()
    two[3, 5] = (const[0, 0].astype(np.int32) + 100) % 256
    cases = [("AutoContrast", (), const), ("Equalize", (), const), ("AutoContrast", (), two), ("Equalize", (), two),
             ("Posterize", (0,), None), ("Posterize", (4,), None), ("Solarize", (0,), None), ("Solarize", (256,), None),
             ("SolarizeAdd", (0,), None), ("SolarizeAdd", (128,), None), ("Invert", (), None), ("Rotate", (0.0,), None)]
    images = []
    for k, (name, args, a) in enumerate(cases):
        ra.put(k, 0, ra.record(name, *args))
        images.append(_image(rng, 24, 40, 0) if a is None else a)
    got, want = _run(ra, images), _want(ra, images)
    assert torch.equal(got, want), _mismatch(ra, got, want)
    src = _planar(images)
    assert torch.equal(got[0], src[0]) and torch.equal(got[1], src[1]) and torch.equal(got[7], src[7])
    assert torch.equal(got[4], torch.zeros_like(got[4])) and torch.equal(got[6], 255 - src[6])


@pytest.mark.parametrize("size", [(24, 40), (40, 24), (37, 41)], ids=["24x40", "40x24", "37x41"])
def test_affine_arguments_that_push_most_of_the_image_out(size):
    from fastvim_amd.randaug import K_AFFINE, Record
    ra = _ra(size, 14, "rand-n1")
    rng = np.random.default_rng(70)
    H, W = size
    ops = [("TranslateXRel", 0.9), ("TranslateXRel", -0.9), ("TranslateYRel", 0.95), ("TranslateYRel", -2.0),
           ("ShearX", 3.0), ("ShearY", -3.0), ("Rotate", 89.0), ("Rotate", -45.0), ("Rotate", 333.3), ("ShearX", 0.0),
           ("TranslateXRel", 0.45), ("TranslateYRel", -0.45)]
    for k, (name, v) in enumerate(ops):
        ra.put(k, 0, ra.record(name, v))
    # a 3x zoom about a corner and a mirrored map: taps clamp at every border
    ra.put(12, 0, Record(K_AFFINE, 0, 0, 1.0, ra.fill, (1 / 3, 0.0, -1.0, 0.0, 1 / 3, -1.0)))
    ra.put(13, 0, Record(K_AFFINE, 0, 0, 1.0, ra.fill, (-1.0, 0.0, W + 0.25, 0.0, -1.0, H - 0.25)))
    images = [_image(rng, H, W, kind=k) for k in range(14)]
    got, want = _run(ra, images), _want(ra, images)
    assert torch.equal(got, want), _mismatch(ra, got, want)
    fill = torch.tensor(ra.fill, dtype=torch.uint8).view(3, 1, 1)
    assert torch.equal(got[3], fill.expand(3, H, W))                 # everything out: the fill colour
    assert (got[0] == fill).all(0).float().mean() > 0.8


def test_pil_fixtures_on_the_device():
    z = np.load(os.path.join(GOLDEN, "randaug_pil.npz"))
    names, args, image = [str(n) for n in z["names"]], z["args"], z["image"]
    for i in range(6):
        a = z[f"src_{i}"]
        ks = [k for k in range(len(names)) if image[k] == i]
        ra = _ra(a.shape[:2], len(ks), "rand-n1")
        for j, k in enumerate(ks):
            ar = () if np.isnan(args[k]) else ((int(args[k]),) if names[k] in ("Posterize", "Solarize", "SolarizeAdd") else (float(args[k]),))
            ra.put(j, 0, ra.record(names[k], *ar))
        got = _run(ra, [a] * len(ks))
        want = _planar([z[f"out_{k}"] for k in ks])
        assert torch.equal(got, want), [(names[k], args[k]) for j, k in enumerate(ks) if not torch.equal(got[j], want[j])]


def test_graph_replay_of_resample_and_apply_reads_the_plans_of_the_moment():
    from fastvim_amd.resample import ImageStage
    import resample_ref
    rng = np.random.default_rng(80)
    size, B = (24, 40), 6
    stage = ImageStage(B, size, capacity_bytes=1 << 18, slots=1)
    ra = _ra(size, B)
    tmp = torch.zeros(B, 3, *size, dtype=torch.uint8, device="cuda")
    x = torch.zeros_like(tmp)

    def fill(r):
        np.random.seed(90 + r)
        random.seed(95 + r)
        crops = []
        for k in range(B):
            a = _image(rng, 50 + 5 * r + k, 61 - 3 * r, kind=k)
            flip = bool((k + r) & 1)
            stage.put(k, a, flip=flip)
            ra.draw(k)
            crops.append(resample_ref.resample(a, size=size, flip=flip).transpose(1, 2, 0))
        if r == 1:
            ra.put(0, 0, ra.record("Equalize"))
            ra.put(1, 1, ra.record("Rotate", 25.0))
        stage.commit()
        ra.commit()
        return _planar([R.apply_plan(np.ascontiguousarray(c), ra.records[k]) for k, c in enumerate(crops)])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        want = fill(0)
        stage.resample(out=tmp)
        ra.apply(tmp, x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), want)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stage.resample(out=tmp)
        ra.apply(tmp, x)
    wants = []
    for r in (1, 2):
        want = fill(r)
        graph.replay()
        assert torch.equal(x.cpu(), want), r
        wants.append(want)
    assert not torch.equal(wants[0], wants[1])


def test_bad_arguments_raise():
    from fastvim_amd import _lib as L
    ra = _ra((16, 24), 2)
    x = torch.zeros(2, 3, 16, 24, dtype=torch.uint8, device="cuda")
    y = torch.zeros_like(x)
    with pytest.raises(RuntimeError, match="nothing was committed"):
        ra.apply(x, y)
    ra.commit()
    ra.apply(x, y)
    with pytest.raises(ValueError, match="distinct"):
        ra.apply(x, x)
    with pytest.raises(ValueError):
        ra.apply(x.float(), y)
    with pytest.raises(ValueError):
        ra.apply(x, torch.zeros(2, 3, 24, 16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        ra.apply(torch.zeros(2, 3, 24, 16, dtype=torch.uint8, device="cuda").transpose(2, 3), y)
    with pytest.raises(ValueError):
        ra.apply(torch.zeros(3, 3, 16, 24, dtype=torch.uint8, device="cuda"), y)
    with pytest.raises(RuntimeError):
        ra.apply(x.cpu(), y)
    with pytest.raises(IndexError):
        ra.draw(2)
    with pytest.raises(IndexError):
        ra.put(0, 2, ra.record("Invert"))
    lib, st = L.lib(), L.stream_of(x)
    i = L.i32
    plan, ws = L.ptr(ra._plan_dev), L.ptr(ra._ws)
    assert lib.fv_randaug_apply(L.ptr(x), L.ptr(y), plan, ws, i(2), i(16), i(24), i(2), i(2), st) != 0       # layer 2 of 2
    assert lib.fv_randaug_stats(L.ptr(x), plan, ws, i(2), i(16), i(24), i(5), i(0), st) != 0                # five layers
    assert lib.fv_randaug_apply(L.ptr(x), L.ptr(x), plan, ws, i(2), i(16), i(24), i(2), i(0), st) != 0      # in is out
    assert lib.fv_randaug_apply(L.ptr(x), L.ptr(y), plan, ws, i(2), i(4), i(24), i(2), i(0), st) != 0       # a side of 4
    assert b"randaug" in lib.fv_last_error()
    torch.cuda.synchronize()
