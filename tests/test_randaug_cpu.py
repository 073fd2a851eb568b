"""RandAugment, host side (fastvim_amd/randaug.py) and its numpy reference (tests/randaug_ref.py):

* the reference equals PIL itself on every op of both of timm's lists -- random draws of the argument at sizes 8x8, 24x40,
  40x24, 37x41 and 224x224 on random, smooth, few-valued and constant images, exact equality -- and the PIL-written
  fixtures (tests/golden/randaug_pil.npz), which need no PIL;
* ``RandAugment.draw`` consumes numpy's and Python's global generators exactly as a literal transcription of timm's
  ``RandAugment.__call__`` / ``AugmentOp.__call__`` does, and yields the same ops and arguments;
* config keys, level functions, the plan record, the host predicate."""
import importlib.util
import math
import os
import random
import re

import numpy as np
import pytest

import randaug_ref as R
from fastvim_amd import randaug as RA

HERE = os.path.dirname(os.path.abspath(__file__))
MEAN = (0.485, 0.456, 0.406)
FILL = (124, 116, 104)
RECIPE = "rand-m9-mstd0.5-inc1"

NAMES = ("AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "PosterizeIncreasing", "Solarize", "SolarizeIncreasing",
         "SolarizeAdd", "Color", "ColorIncreasing", "Contrast", "ContrastIncreasing", "Brightness", "BrightnessIncreasing",
         "Sharpness", "SharpnessIncreasing", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")


def _ra(size, config=RECIPE, batch=1):
    return RA.RandAugment(config, size, MEAN, batch)


def _images(rng, H, W):
    """random, smooth (blurred), few-valued and constant images of one size"""
    a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    s = rng.integers(0, 256, (H + 4, W + 4, 3)).astype(np.float64)
    for _ in range(2):
        s = (s + np.roll(s, 1, 0) + np.roll(s, -1, 0) + np.roll(s, 1, 1) + np.roll(s, -1, 1)) / 5
    s = s[2:-2, 2:-2].round().astype(np.uint8)
    few = (rng.integers(0, 3, (H, W, 3)) * 100 + 20).astype(np.uint8)
    const = np.broadcast_to(rng.integers(0, 256, 3).astype(np.uint8), (H, W, 3)).copy()
    return [a, s, few, const]


# ------------------------------------------------------------------------------------------------- reference against PIL
@pytest.fixture(scope="module")
def pil_op():
    pytest.importorskip("PIL")
    spec = importlib.util.spec_from_file_location("gen_randaug", os.path.join(HERE, "golden", "gen_randaug.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.pil_op


SIZES = [(8, 8), (24, 40), (40, 24), (37, 41)]


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_pil(name, pil_op):
    """304 draws per op name on small images (4 sizes x 4 image types x 19 arguments) and 6 at 224 x 224: the argument from
    timm's level function at a magnitude drawn as the recipe draws it (gauss(9, 0.5)), uniformly in [0, 10], or an end."""
    from PIL import Image
    rng = np.random.default_rng(NAMES.index(name))
    random.seed(1000 + NAMES.index(name))
    n = 0
    plans = [(s, 19) for s in SIZES] + [((224, 224), 2)]
    for (H, W), reps in plans:
        ra = _ra((H, W))
        imgs = _images(rng, H, W)
        for a in (imgs if H < 224 else imgs[:3]):
            for r in range(reps):
                mag = (random.gauss(9, 0.5), random.uniform(0, 10), 0.0, 10.0)[r % 4 if r < 16 else 0]
                mag = max(0., min(mag, 10.))
                args = ra.level_args(name, mag)
                want = np.asarray(pil_op(name, Image.fromarray(a), args, FILL))
                got = R.apply_record(a, ra.record(name, *args))
                assert np.array_equal(got, want), (name, args, (H, W), int((got != want).sum()))
                n += 1
    assert n >= 300


def test_reference_equals_pil_equalize_clips_above_255(pil_op):
    """A 224 x 224 image whose equalize table has entries of 256 before the clip (they must not wrap to 0)."""
    from PIL import Image
    a = R.equalize_overflow_image()
    for h in R.histogram(a):
        step = (int(h.sum()) - int(h[np.nonzero(h)[0][-1]])) // 255
        assert (step // 2 + int(h[:255].sum())) // step == 256 and R.equalize_lut(h)[255] == 255
    want = np.asarray(pil_op("Equalize", Image.fromarray(a)))
    assert np.array_equal(R.apply_record(a, _ra(224).record("Equalize")), want)


def test_reference_equals_the_pil_fixtures():
    z = np.load(os.path.join(HERE, "golden", "randaug_pil.npz"))
    names, args, image = z["names"], z["args"], z["image"]
    assert len(names) >= 200 and set(RA.OPS) <= set(str(n) for n in names)
    assert tuple(int(v) for v in z["fill"]) == FILL
    for k, (name, arg, i) in enumerate(zip(names, args, image)):
        name, a = str(name), z[f"src_{int(i)}"]
        ar = () if math.isnan(arg) else ((int(arg),) if name in ("Posterize", "Solarize", "SolarizeAdd") else (float(arg),))
        got = R.apply_record(a, _ra(a.shape[:2]).record(name, *ar))
        assert np.array_equal(got, z[f"out_{k}"]), (k, name, ar, a.shape)


# ------------------------------------------------------------------------------------------------------- the draw stream
def _timm_level(name, level):
    """timm's level functions, transcribed (``_LEVEL_DENOM = 10.``, translate_pct 0.45)."""
    def negate(v):
        return -v if random.random() > 0.5 else v
    if name in ("AutoContrast", "Equalize", "Invert"):
        return ()
    if name == "Rotate":
        return (negate((level / 10.) * 30.),)
    if name in ("ShearX", "ShearY"):
        return (negate((level / 10.) * 0.3),)
    if name in ("TranslateXRel", "TranslateYRel"):
        return (negate((level / 10.) * 0.45),)
    if name in ("Color", "Contrast", "Brightness", "Sharpness"):
        return ((level / 10.) * 1.8 + 0.1,)
    if name in ("ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing"):
        return (max(0.1, 1.0 + negate((level / 10.) * .9)),)
    if name == "Posterize":
        return (int((level / 10.) * 4),)
    if name == "PosterizeIncreasing":
        return (4 - int((level / 10.) * 4),)
    if name == "Solarize":
        return (min(256, int((level / 10.) * 256)),)
    if name == "SolarizeIncreasing":
        return (256 - min(256, int((level / 10.) * 256)),)
    if name == "SolarizeAdd":
        return (min(128, int((level / 10.) * 110)),)
    raise AssertionError(name)


def _timm_draw(config_str):
    """``rand_augment_transform(config_str, ...)`` then ``RandAugment.__call__`` of one image, without the pixels."""
    magnitude, num_layers, prob, mstd, mmax, increasing = 10, 2, 0.5, 0.0, None, False
    for c in config_str.split("-")[1:]:
        cs = re.split(r"(\d.*)", c)
        if len(cs) < 2:
            continue
        key, val = cs[:2]
        if key == "mstd":
            mstd = float(val)
            if mstd > 100:
                mstd = float("inf")
        elif key == "mmax":
            mmax = int(val)
        elif key == "inc":
            if bool(val):
                increasing = True
        elif key == "m":
            magnitude = int(val)
        elif key == "n":
            num_layers = int(val)
        elif key == "p":
            prob = float(val)
        else:
            raise AssertionError(key)
    names = list(RA.OPS_INCREASING if increasing else RA.OPS)
    out = []
    for name in np.random.choice(names, num_layers, replace=True, p=None):
        if prob < 1.0 and random.random() > prob:
            out.append((None, ()))
            continue
        m = magnitude
        if mstd == float("inf"):
            m = random.uniform(0, m)
        elif mstd > 0:
            m = random.gauss(m, mstd)
        m = max(0., min(m, mmax or 10.))
        out.append((str(name), _timm_level(str(name), m)))
    return out


CONFIGS = [RECIPE, "rand-m9-mstd0.5", "rand-m7-mstd101-inc1", "rand-m9-mstd0.5-mmax8-inc1", "rand-m9-n3-mstd0.5-inc1",
           "rand-m9-mstd0.5-p1.0-inc1", "rand-m5-n4-p0.3"]


@pytest.mark.parametrize("config", CONFIGS)
def test_draw_consumes_the_generators_as_timm_does(config):
    np.random.seed(11)
    random.seed(12)
    want = [_timm_draw(config) for _ in range(64)]
    state = (np.random.get_state(), random.getstate())
    np.random.seed(11)
    random.seed(12)
    ra = _ra((24, 40), config, batch=64)
    got = [ra.draw(k) for k in range(64)]
    assert got == want
    s = np.random.get_state()
    assert s[0] == state[0][0] and np.array_equal(s[1], state[0][1]) and s[2:] == state[0][2:]
    assert random.getstate() == state[1]
    kinds = {n for layers in got for n, _ in layers}
    assert len(kinds) >= 10
    if "p1.0" in config:
        assert None not in kinds
    else:
        assert None in kinds
    # the records the draw left in the plan are those of the drawn ops
    for k, layers in enumerate(got):
        assert len(layers) == ra.num_layers
        for l, (name, args) in enumerate(layers):
            rec = ra.record("Identity") if name is None else ra.record(name, *args)
            assert np.array_equal(ra.plan[k, l], RA.pack_record(rec))
            assert ra.records[k][l] == rec


def test_config_keys_and_level_functions():
    ra = _ra(224)
    assert (ra.magnitude, ra.num_layers, ra.prob, ra.magnitude_std, ra.magnitude_max) == (9, 2, 0.5, 0.5, None)
    assert ra.names == RA.OPS_INCREASING and ra.fill == FILL
    assert _ra(224, "rand-m9-mstd0.5").names == RA.OPS
    assert _ra(224, "rand-m9-inc0").names == RA.OPS_INCREASING            # bool('0') is True, as in timm
    assert _ra(224, "rand-mstd101").magnitude_std == float("inf") and _ra(224, "rand-mstd100").magnitude_std == 100.0
    r4 = _ra(224, "rand-m3-n4-p0.25-mmax20")
    assert (r4.magnitude, r4.num_layers, r4.prob, r4.magnitude_max, r4.upper_bound) == (3, 4, 0.25, 20, 20)
    assert _ra(224, "rand").magnitude == 10
    for bad in ("rand-m9-w0", "rand-t1-m9"):
        with pytest.raises(NotImplementedError):
            _ra(224, bad)
    with pytest.raises(ValueError, match="90 degrees"):
        _ra(224, "rand-m9-mmax30")
    _ra(224, "rand-m9-mmax29")
    with pytest.raises(ValueError):
        _ra(224, "rand-m9-n5")
    with pytest.raises(ValueError):
        _ra(224, "rand-m9-q3")
    with pytest.raises(ValueError):
        _ra(224, "augmix-m9")
    for size in (7, 1025, (224, 4)):
        with pytest.raises(ValueError):
            _ra(size)
    # level functions at chosen magnitudes (no sign drawn for these)
    assert ra.level_args("AutoContrast", 9) == ()
    assert ra.level_args("Posterize", 9.9) == (3,) and ra.level_args("Posterize", 10) == (4,)
    assert ra.level_args("PosterizeIncreasing", 10) == (0,) and ra.level_args("PosterizeIncreasing", 0) == (4,)
    assert ra.level_args("Solarize", 10) == (256,) and ra.level_args("Solarize", 5) == (128,)
    assert ra.level_args("SolarizeIncreasing", 9) == (26,) and ra.level_args("SolarizeIncreasing", 0) == (256,)
    assert ra.level_args("SolarizeAdd", 9) == (99,) and ra.level_args("SolarizeAdd", 10) == (110,)
    assert ra.level_args("Color", 0) == (0.1,) and ra.level_args("Sharpness", 10) == (1.8 + 0.1,)
    random.seed(3)
    signs = set()
    for _ in range(40):
        (v,) = ra.level_args("BrightnessIncreasing", 10)
        assert v in (1.9, 0.1)                                     # max(0.1, 1 - 0.9) is the floor 0.1
        (d,) = ra.level_args("Rotate", 9)
        assert abs(d) == 27.0
        (t,) = ra.level_args("TranslateYRel", 10)
        assert abs(t) == 0.45
        signs |= {v, d, t}
    assert len(signs) == 6


def test_records_of_the_geometry():
    ra = _ra((24, 40))
    assert ra.record("Rotate", 0.0).kind == RA.K_COPY and ra.record("Rotate", 360.0).kind == RA.K_COPY
    assert ra.record("Posterize", 8).kind == RA.K_COPY
    deg = 27.0
    a = -math.radians(deg % 360)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0, round(-math.sin(a), 15), round(math.cos(a), 15), 0]
    m[2] = m[0] * (-40 / 2) + m[1] * (-24 / 2) + 40 / 2
    m[5] = m[3] * (-40 / 2) + m[4] * (-24 / 2) + 24 / 2
    assert ra.record("Rotate", deg).coeffs == tuple(m) and ra.record("Rotate", deg).kind == RA.K_AFFINE
    assert ra.record("Rotate", -333.0).coeffs == tuple(m)
    assert ra.record("ShearX", -0.27).coeffs == (1, -0.27, 0, 0, 1, 0)
    assert ra.record("ShearY", 0.3).coeffs == (1, 0, 0, 0.3, 1, 0)
    assert ra.record("TranslateXRel", 0.405).coeffs == (1, 0, 0.405 * 40, 0, 1, 0)
    assert ra.record("TranslateYRel", -0.405).coeffs == (1, 0, 0, 0, 1, -0.405 * 24)
    assert ra.record("SolarizeAdd", 99)[:3] == (RA.K_SOLARIZE_ADD, 99, 128)
    assert ra.record("ColorIncreasing", 1.81) == ra.record("Color", 1.81)


def test_plan_record_round_trip():
    ra = _ra((37, 41))
    rng = np.random.default_rng(0)
    recs = [ra.record("Rotate", 26.123456789), ra.record("ShearX", -0.1 / 3), ra.record("TranslateYRel", 0.45),
            ra.record("Sharpness", 1.72), ra.record("Solarize", 230), ra.record("SolarizeAdd", 99), ra.record("Equalize"),
            RA.Record(RA.K_AFFINE, -5, 2 ** 31 - 1, 0.1, (255, 0, 128), tuple(float(v) for v in rng.standard_normal(6) * 1e3)),
            RA.Record(RA.K_AFFINE, 0, 0, 1.0, (0, 0, 0), (5e-324, -0.0, 1.7976931348623157e308, math.pi, -1e-300, 1 / 3))]
    for rec in recs:
        w = RA.pack_record(rec)
        assert w.dtype == np.int32 and w.shape == (RA.PLAN_INTS,)
        back = RA.unpack_record(w)
        assert back[:3] == rec[:3] and back.fill == tuple(rec.fill)
        assert np.float32(back.factor) == np.float32(rec.factor) and back.factor == float(np.float32(rec.factor))
        assert np.array(back.coeffs).tobytes() == np.array(rec.coeffs, np.float64).tobytes()      # bit for bit
        assert w[6:].tobytes() == np.array(rec.coeffs, "<f8").tobytes() and w[5] == 0
        assert np.array_equal(RA.pack_record(back), w)
    w = RA.pack_record(recs[3])
    assert w[3] == np.array([1.72], np.float32).view(np.int32)[0]
    assert w[4] == 124 | (116 << 8) | (104 << 16)


def test_host_predicate_agrees_with_the_library():
    import fastvim_amd.build as fb
    fb.build()
    for batch in (0, 1, 4096, 4097):
        for sh in (7, 8, 1024, 1025):
            for sw in (7, 8, 37, 1024, 1025):
                for nl in (0, 1, 4, 5):
                    assert RA.randaug_ok(batch, sh, sw, nl) == RA.served(batch, sh, sw, nl), (batch, sh, sw, nl)
    from fastvim_amd import _lib as L
    assert int(L.lib().fv_randaug_workspace_bytes(L.i32(7))) == 7 * RA.WS_BYTES


def test_apply_has_no_cpu_form():
    import torch
    ra = _ra(16, batch=2)
    x = torch.zeros(2, 3, 16, 16, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        ra.apply(x, x.clone())
    assert not hasattr(ra, "apply_host")
