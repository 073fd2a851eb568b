"""The numpy restatement of the device-side cell augmentation (tests/cellaug_ref.py) against independent arithmetic on the
CPU, and the host half of fastvim_amd/cellaug.py (draws, matrix and kernel construction, record layout, refusals).

OpenCV is not a dependency, so the restatement is the contract the GPU tests compare bytes against; here it is tied to
scipy.ndimage in fp64 within bounds that are derived, not fitted:

* rotation: coordinates are quantised to 1/32 pixel after two roundings to 1/1024, so each of the two axes is off by at
  most 1/64 + 1/1024 pixel; on a fixture whose neighbouring pixels differ by at most 12 the bilinear value moves by at most
  2 * 12 * (1/64 + 1/1024) = 0.40, the output rounding adds 0.5: below 0.9, asserted as < 1.0.
* defocus: fp32 accumulation of 81 non-negative products below 255 is within 1e-3 of the fp64 sum, so the bytes are
  equal wherever the fp64 value is farther than 1e-3 from a half-integer; those are under 1 % of the pixels."""
import math

import numpy as np
import pytest
from scipy import ndimage

import cellaug_ref as R
from fastvim_amd import cellaug as CA

ANGLES = (-270.0, -180.0, -133.7, -90.0, -45.0, -17.3, 0.0, 17.3, 45.0, 90.0, 133.7, 180.0, 270.0)
SHAPES = ((16, 16), (24, 40), (33, 17))


def _smooth(h, w):
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    img = np.rint(128 + 60 * np.sin(x / 5 + 1) + 50 * np.cos(y / 6 - 1)).astype(np.uint8)
    assert np.abs(np.diff(img.astype(int), axis=0)).max() <= 12 and np.abs(np.diff(img.astype(int), axis=1)).max() <= 12
    return img


# ------------------------------------------------------------------------------------------------------------- rotation
@pytest.mark.parametrize("shape", SHAPES)
def test_rotation_against_scipy(shape):
    h, w = shape
    img = _smooth(h, w)
    worst = 0.0
    for angle in ANGLES:
        m = R.rotation_matrix(h, w, angle)
        got = R.warp(img, m).astype(np.float64)
        # scipy indexes (row, col): row = m4 y + m3 x + m5, col = m1 y + m0 x + m2
        want = ndimage.affine_transform(img.astype(np.float64), np.array([[m[4], m[3]], [m[1], m[0]]]), offset=(m[5], m[2]),
                                        order=1, mode="mirror")
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"rotation {h}x{w}: max |restatement - scipy| = {worst:.3f}")
    assert worst < 1.0


@pytest.mark.parametrize("shape", SHAPES)
def test_rotation_by_zero_is_the_identity(shape):
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    assert np.array_equal(R.warp(img, R.rotation_matrix(*shape, 0.0)), img)


def test_rotation_by_180_is_the_point_mirror_within_the_bound():
    img = _smooth(16, 16)
    got = R.warp(img, R.rotation_matrix(16, 16, 180.0)).astype(int)
    assert np.abs(got - img[::-1, ::-1].astype(int)).max() < 1.0 + 1e-9


def test_host_matrix_is_the_restatements():
    for size in (16, 40, 224):
        for angle in ANGLES:
            assert CA.rotation_matrix(size, angle) == R.rotation_matrix(size, size, angle)
    m = CA.rotation_matrix(224, 90.0)
    # the inverse of a rotation by +90 degrees (counter-clockwise on the screen): sx = 223 - y, sy = x
    assert np.allclose(m, (0, -1, 223, 1, 0, 0), atol=1e-9)


# -------------------------------------------------------------------------------------------------------------- defocus
def test_defocus_against_scipy():
    rng = np.random.default_rng(1)
    total = left_out = 0
    for radius in (1, 2, 3):
        for sigma in (0.1, 0.3, 0.5):
            full = R.defocus_kernel_full(radius, sigma)
            k9 = R.defocus_kernel(radius, sigma)
            assert full.shape == (17, 17) and k9.shape == (9, 9) and full.dtype == np.float32
            for shape in ((8, 8), (16, 24), (37, 19)):
                plane = rng.integers(0, 256, shape, dtype=np.uint8)
                got = R.correlate(plane, k9)
                want = ndimage.correlate(plane.astype(np.float64), full.astype(np.float64), mode="mirror")
                clear = np.abs(want - np.floor(want) - 0.5) > 1e-3
                assert np.array_equal(got[clear], np.clip(np.rint(want), 0, 255).astype(np.uint8)[clear]), (radius, sigma, shape)
                total += plane.size
                left_out += int((~clear).sum())
    print(f"defocus: {left_out} of {total} pixels within 1e-3 of a half-integer ({100.0 * left_out / total:.2f} %)")
    assert left_out < 0.01 * total


@pytest.mark.parametrize("radius", (1, 2, 3))
@pytest.mark.parametrize("sigma", (0.1, 0.25, 0.5))
def test_defocus_kernel_support_and_sum(radius, sigma):
    full = CA.defocus_kernel_full(radius, sigma)
    assert np.array_equal(full, R.defocus_kernel_full(radius, sigma))
    assert np.array_equal(CA.defocus_kernel(radius, sigma), R.defocus_kernel(radius, sigma))
    ys, xs = np.nonzero(full)
    assert np.abs(ys - 8).max() <= radius + 1 and np.abs(xs - 8).max() <= radius + 1
    assert (full >= 0).all()
    # 81 fp32 entries, each rounded a handful of times: within 81 * 4 ulp of 1
    assert abs(float(full.astype(np.float64).sum()) - 1.0) < 81 * 4 * 2.0 ** -24


def test_defocus_radius_above_three_raises():
    with pytest.raises(ValueError, match="radius"):
        CA.defocus_kernel(4, 0.3)
    with pytest.raises(ValueError, match="radius"):
        CA.CellAugmentation(224, radius=(1, 4))
    host = CA.HostCellPlan(1, 1, 16, 4096)
    with pytest.raises(ValueError, match="radius"):
        host.put(0, np.zeros((1, 16, 16), np.uint8), CA.CellPlan(radius=4, sigma=0.2))


# ----------------------------------------------------------------------------------------- pad, crop, flips and holes
@pytest.mark.parametrize("hw", ((9, 13), (50, 37), (16, 16)))
def test_pad_crop_flips_against_slicing(hw):
    rng = np.random.default_rng(2)
    S, (h, w) = 16, hw
    src = rng.integers(1, 256, (3, h, w), dtype=np.uint8)
    for pad_top, pad_left, crop_top, crop_left in ((0, 0, 0, 0), (5, 3, 2, 1), (2, 1, 7, 9), (40, 40, 30, 35), (0, 0, 40, 30)):
        canvas = np.zeros((3, 128, 128), np.uint8)
        canvas[:, pad_top:pad_top + h, pad_left:pad_left + w] = src
        crop = canvas[:, crop_top:crop_top + S, crop_left:crop_left + S]
        oy, ox = pad_top - crop_top, pad_left - crop_left
        assert np.array_equal(R.geom(src, S, oy, ox), crop)
        assert np.array_equal(R.geom(src, S, oy, ox, R.HFLIP), crop[:, :, ::-1])
        assert np.array_equal(R.geom(src, S, oy, ox, R.VFLIP), crop[:, ::-1, :])
        # a rotation by 0 degrees goes through the tap arithmetic and still is the crop
        assert np.array_equal(R.geom(src, S, oy, ox, R.ROTATE, R.rotation_matrix(S, S, 0.0)), crop)
        # and by an angle it is the warp of the crop: padding zeros reflect like any other pixel
        m = R.rotation_matrix(S, S, 33.0)
        assert np.array_equal(R.geom(src, S, oy, ox, R.ROTATE, m), R.warp(crop, m))


def test_holes_against_slicing():
    rng = np.random.default_rng(3)
    planes = rng.integers(1, 256, (2, 16, 16), dtype=np.uint8)
    holes = ((0, 0, 3, 4), (10, 12, 16, 16), (5, 5, 5, 9))          # on two borders; the last one is empty
    want = planes.copy()
    want[:, 0:3, 0:4] = 0
    want[:, 10:16, 12:16] = 0
    assert np.array_equal(R.filter(planes, None, holes), want)
    assert np.array_equal(R.filter(planes, None, ()), planes)
    k = R.defocus_kernel(2, 0.3)
    blurred = R.filter(planes, k, holes)
    full = R.correlate(planes, k)
    assert (blurred[:, 0:3, 0:4] == 0).all() and np.array_equal(blurred[:, 4:10], full[:, 4:10])


# ----------------------------------------------------------------------------------------------------------------- draw
def test_draw_is_reproducible():
    a, b, c = CA.CellAugmentation(224, seed=7), CA.CellAugmentation(224, seed=7), CA.CellAugmentation(224, seed=8)
    sizes = [(100 + 7 * k % 90, 80 + 11 * k % 120) for k in range(200)]
    pa, pb, pc = ([aug.draw(h, w) for h, w in sizes] for aug in (a, b, c))
    assert pa == pb and pa != pc


def test_draw_ranges_and_frequencies():
    S, n = 224, 20000
    aug = CA.CellAugmentation(S, seed=11)
    rng = np.random.default_rng(4)
    fired = np.zeros(3)
    members = np.zeros(5)
    for _ in range(n):
        h, w = int(rng.integers(40, 400)), int(rng.integers(40, 400))
        p = aug.draw(h, w)
        canvas_h, canvas_w = max(256, h), max(256, w)
        # oy = pad_top - crop_top with pad_top in [0, canvas - h] and crop_top in [0, canvas - S]
        assert -(canvas_h - S) <= p.oy <= canvas_h - h and -(canvas_w - S) <= p.ox <= canvas_w - w
        assert p.op in (CA.NONE, CA.HFLIP, CA.VFLIP, CA.ROTATE)
        if p.op != CA.NONE:
            fired[0] += 1
            assert -270.0 <= p.angle <= 270.0 if p.op == CA.ROTATE else p.angle == 0.0
        if p.radius:
            fired[1] += 1
            assert 1 <= p.radius <= 3 and 0.1 <= p.sigma <= 0.5
        else:
            assert p.sigma == 0.0
        if p.holes:
            fired[2] += 1
            assert len(p.holes) == 10
            for y1, x1, y2, x2 in p.holes:
                assert 0 <= y1 and y2 <= S and 0 <= x1 and x2 <= S and y2 - y1 == 10 and x2 - x1 == 10
    assert np.abs(fired / n - 0.5).max() < 0.02, fired / n

    # the five OneOf members: a rotation's member is not kept in the plan, so the documented order is replayed on a second
    # generator with the same seed, which must end in the same state
    import random
    aug = CA.CellAugmentation(S, seed=12, p_defocus=0.0, p_dropout=0.0)
    stream = random.Random(12)
    for _ in range(n):
        aug.draw(256, 256)
        stream.randint(0, 0), stream.randint(0, 0)                       # pad top, left
        stream.randint(0, 256 - S), stream.randint(0, 256 - S)           # crop top, left
        if stream.random() < 0.5:
            m = stream.randrange(5)
            members[m] += 1
            if m >= 2:
                stream.uniform(-1, 1)
        stream.random(), stream.random()                                 # defocus and dropout do not fire
    assert aug.rng.getstate() == stream.getstate(), "draw() does not consume its generator in the documented order"
    assert np.abs(members / members.sum() - 0.2).max() < 0.02, members / members.sum()


def test_draw_keywords():
    aug = CA.CellAugmentation(64, seed=0, p_flip_rotate=1.0, p_defocus=1.0, p_dropout=1.0, max_holes=6, min_holes=2,
                              max_height=8, min_height=3, max_width=5, min_width=5, radius=(2, 2), alias_blur=(0.2, 0.2),
                              rotate_limits=(10, 20, 30))
    seen = set()
    for _ in range(300):
        p = aug.draw(70, 300)
        assert p.op != CA.NONE and p.radius == 2 and p.sigma == 0.2 and 2 <= len(p.holes) <= 6
        assert abs(p.angle) <= 30
        seen.add(len(p.holes))
        for y1, x1, y2, x2 in p.holes:
            assert 3 <= y2 - y1 <= 8 and x2 - x1 == 5 and y2 <= 64 and x2 <= 64
    assert seen == {2, 3, 4, 5, 6}
    quiet = CA.CellAugmentation(64, seed=0, p_flip_rotate=0.0, p_defocus=0.0, p_dropout=0.0)
    p = quiet.draw(64, 64)
    assert (p.op, p.radius, p.holes) == (CA.NONE, 0, ())
    with pytest.raises(ValueError, match="canvas"):
        CA.CellAugmentation(300, seed=0).draw(100, 100)
    with pytest.raises(ValueError, match="holes"):
        CA.CellAugmentation(64, max_holes=17)


# ------------------------------------------------------------------------------------------------------- the host half
def test_record_round_trip():
    rng = np.random.default_rng(5)
    host = CA.HostCellPlan(3, 2, 16, 8192)
    imgs = [rng.integers(0, 256, (2, 9, 13), dtype=np.uint8), rng.integers(0, 256, (2, 50, 37), dtype=np.uint8),
            rng.integers(0, 256, (2, 16, 16), dtype=np.uint8)]
    plans = [CA.CellPlan(3, -2, CA.ROTATE, -133.7, 3, 0.25, ((0, 0, 4, 4), (12, 10, 16, 16))), CA.CellPlan(-20, -11, CA.VFLIP), None]
    offs = [host.put(k, imgs[k], plans[k]) for k in (1, 0, 2)]
    assert offs == [0, 3712, 3712 + 240] and all(o % CA.ALIGN == 0 for o in offs)          # 2*50*37 = 3700 -> 3712; 2*9*13 = 234 -> 240
    host.check_complete()
    assert host.used == 3952 + 512
    for k in range(3):
        off, h, w, oy, ox, op, matrix, kernel, holes = CA.read_record(host.plan[k])
        p = plans[k] or CA.CellPlan()
        assert (h, w) == imgs[k].shape[1:] and (oy, ox, op, holes) == (p.oy, p.ox, p.op, p.holes)
        assert np.array_equal(host.pool[off:off + imgs[k].size].reshape(imgs[k].shape), imgs[k])
        if p.op == CA.ROTATE:
            assert matrix == R.rotation_matrix(16, 16, p.angle)
        else:
            assert matrix == (0.0,) * 6
        if p.radius:
            assert np.array_equal(kernel, R.defocus_kernel(p.radius, p.sigma))
        else:
            assert kernel is None
    # the documented word positions, read without the helper
    row = host.plan[0]
    assert tuple(row[2:9]) == (9, 13, 3, -2, CA.ROTATE, 1, 2) and tuple(row[9:12]) == (0, 0, 0)
    assert row[12:24].view(np.float64)[0] == R.rotation_matrix(16, 16, -133.7)[0]
    assert row[24:105].view(np.float32)[40] == R.defocus_kernel(3, 0.25)[4, 4]
    assert tuple(row[108:116]) == (0, 0, 4, 4, 12, 10, 16, 16) and not row[116:].any()
    assert host.plan.shape[1] == CA.PLAN_INTS == 176


def test_refusals():
    host = CA.HostCellPlan(2, 3, 16, 1000)
    ok = np.zeros((3, 16, 16), np.uint8)
    with pytest.raises(ValueError, match="uint8"):
        host.put(0, ok.astype(np.float32), CA.CellPlan())
    with pytest.raises(ValueError, match="uint8"):
        host.put(0, ok[0], CA.CellPlan())
    with pytest.raises(ValueError, match="channels"):
        host.put(0, np.zeros((8, 16, 16), np.uint8), CA.CellPlan())
    with pytest.raises(ValueError, match="without a plan"):
        host.put(0, np.zeros((3, 16, 17), np.uint8), None)
    with pytest.raises(IndexError):
        host.put(2, ok, None)
    with pytest.raises(ValueError, match="holes"):
        host.put(0, ok, CA.CellPlan(holes=[(0, 0, 1, 1)] * 17))
    with pytest.raises(ValueError, match="hole"):
        host.put(0, ok, CA.CellPlan(holes=[(0, 0, 17, 1)]))
    with pytest.raises(ValueError, match="sigma"):
        host.put(0, ok, CA.CellPlan(radius=2, sigma=0.0))
    with pytest.raises(ValueError, match="angle"):
        host.put(0, ok, CA.CellPlan(op=CA.ROTATE, angle=float("nan")))
    assert host.filled == [False, False] and host.used == 0                    # a refused put leaves nothing behind
    host.put(0, ok, None)
    with pytest.raises(ValueError, match="already put"):
        host.put(0, ok, None)
    with pytest.raises(ValueError, match="overflows"):
        host.put(1, ok, None)                                                  # 768 + 768 > 1000
    with pytest.raises(RuntimeError, match="never put"):
        host.check_complete()
    for bad in (dict(batch=0), dict(batch=4097), dict(channels=0), dict(channels=17), dict(out_size=7), dict(out_size=513)):
        kw = dict(batch=2, channels=3, out_size=16, capacity_bytes=64)
        kw.update(bad)
        with pytest.raises(ValueError, match="range"):
            CA.HostCellPlan(**kw)
    with pytest.raises(ValueError, match="4096"):
        CA.HostCellPlan(1, 1, 16, 1 << 16).put(0, np.zeros((1, 1, 4097), np.uint8), CA.CellPlan())
    # no CPU form of the launches
    import torch
    with pytest.raises(RuntimeError, match="GPU"):
        CA.CellStage(1, channels=1, out_size=16, capacity_bytes=256, device="cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        CA.geom(torch.zeros(256, dtype=torch.uint8), torch.zeros(1, CA.PLAN_INTS, dtype=torch.int32),
                torch.zeros(1, 1, 16, 16, dtype=torch.uint8))


def test_plan_math_is_finite_for_every_drawn_angle():
    aug = CA.CellAugmentation(224, seed=3, p_flip_rotate=1.0)
    for _ in range(500):
        p = aug.draw(200, 200)
        if p.op == CA.ROTATE:
            m = CA.rotation_matrix(224, p.angle)
            assert all(math.isfinite(v) for v in m) and abs(m[0] * m[4] - m[1] * m[3] - 1.0) < 1e-12
