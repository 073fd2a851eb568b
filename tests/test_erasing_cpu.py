"""Host side of random erasing (fastvim_amd/erasing.py), no GPU: the reference's Philox against known answers, the box
draws against the independent restatement in tests/erase_ref.py (same boxes, same consumption of Python's ``random``), the
erase block's bytes, the counter and the refusals."""
import random
import struct

import pytest

import erase_ref as R

SIZES = [(224, 224), (448, 448), (32, 40)]


def _re(*a, **kw):
    from fastvim_amd.erasing import RandomErasing
    return RandomErasing(*a, **kw)


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert " ".join(f"{w:08x}" for w in R.philox4x32_10(ctr, key)) == want
        got = R.philox4x32_10_np(*[[c] for c in ctr], key)
        assert " ".join(f"{int(w[0]):08x}" for w in got) == want


def test_scalar_and_array_noise_agree_and_pairs_share_a_group():
    key = (0x12345678, 0x9abcdef0)
    box = R.noise_box(key, 3, 2, 5, 3, 4, 7)
    for c in range(2):
        for y in range(4):
            for x in range(7):
                assert box[c, y, x] == R.noise_at(key, 3, c, 5 + y, 3 + x)
    # pixels 4..7 of a row come from ONE Philox call: words 0, 1 -> (cos, sin), words 2, 3 -> (cos, sin)
    r = R.philox4x32_10((1, 9, 0, 0), key)
    z = R.box_muller(r[0], r[1])
    assert (R.noise_at(key, 0, 0, 9, 4), R.noise_at(key, 0, 0, 9, 5)) == (float(z[0]), float(z[1]))
    z = R.box_muller(r[2], r[3])
    assert (R.noise_at(key, 0, 0, 9, 6), R.noise_at(key, 0, 0, 9, 7)) == (float(z[0]), float(z[1]))


@pytest.mark.parametrize("prob", [0.25, 1.0])
@pytest.mark.parametrize("H,W", SIZES)
def test_sample_draws_the_reference_boxes_and_consumes_the_same_stream(H, W, prob):
    B = 2000
    for k in (0, 1, 7):
        re = _re(prob, mode="pixel", max_count=1).bind((B, 3, H, W))
        random.seed(k)
        got = re.sample()
        state = random.getstate()
        random.seed(k)
        want = R.draw_boxes(random, B, H, W, prob)
        assert got == want == re.last()
        assert random.getstate() == state
        n = 0
        for top, left, h, w in got:
            if (top, left, h, w) == (0, 0, 0, 0):
                continue
            n += 1
            assert 0 < h < H and 0 < w < W and 0 <= top and 0 <= left and top + h <= H and left + w <= W
        assert n == B if prob == 1.0 else 0.18 * B < n < 0.32 * B
        # an explicit generator is used instead of the module's, which is left alone
        random.seed(99)
        before = random.getstate()
        assert re.sample(rng=random.Random(k)) == want and random.getstate() == before


def test_other_constructor_arguments_reach_the_draw():
    re = _re(1.0, min_area=0.1, max_area=0.2, min_aspect=0.5, max_aspect=3.0, mode="const").bind((500, 3, 64, 96))
    random.seed(4)
    got = re.sample()
    random.seed(4)
    assert got == R.draw_boxes(random, 500, 64, 96, 1.0, 0.1, 0.2, 0.5, 3.0)
    assert all(0.08 * 64 * 96 < h * w < 0.22 * 64 * 96 for _, _, h, w in got)


def test_packed_block_round_trips_and_counter_advances_once_per_sample():
    from fastvim_amd.erasing import derive_key
    re = _re(1.0, mode="pixel", seed=5).bind((3, 3, 32, 40))
    assert re.counter == 0 and re.last() == [(0, 0, 0, 0)] * 3
    words = struct.unpack("<IIii12i", re.packed())
    assert words[:2] == derive_key(5, 0) and words[2:4] == (1, 3) and words[4:] == (0,) * 12
    boxes = re.sample(rng=random.Random(0))
    assert re.counter == 1
    words = struct.unpack("<IIii12i", re.packed())
    assert len(re.packed()) == 4 * (4 + 4 * 3)
    assert words[:2] == derive_key(5, 1) == re.key() and words[2:4] == (1, 3)
    assert [tuple(words[4 + 4 * b: 8 + 4 * b]) for b in range(3)] == boxes
    re.set([None, (1, 2, 3, 4), (0, 0, 0, 0)])
    assert re.counter == 1 and re.key() == derive_key(5, 1)                   # set() keeps the key
    assert struct.unpack("<IIii12i", re.packed())[4:] == (0, 0, 0, 0, 1, 2, 3, 4, 0, 0, 0, 0)
    re.sample(rng=random.Random(0))
    assert re.counter == 2
    assert struct.unpack("<IIii", _re(0.5, mode="const").bind((1, 3, 8, 8)).packed()[:16])[2] == 0
    # keys: all different over seeds and counters (ranks pass different seeds)
    keys = {derive_key(s, c) for s in range(8) for c in range(64)}
    assert len(keys) == 8 * 64 and all(0 <= k0 < 2 ** 32 and 0 <= k1 < 2 ** 32 for k0, k1 in keys)


def test_set_validates_its_input():
    re = _re(0.5).bind((2, 3, 32, 40))
    for bad in ([(0, 0, 4, 4)], [(0, 0, 4, 4)] * 3,                       # wrong count
                [(0, 0, 4, 4), (30, 0, 3, 4)], [(0, 38, 4, 3), None],      # past the bottom / the right edge
                [(-1, 0, 4, 4), None], [(0, 0, -4, 4), None], [(0, 0, 4), None]):
        with pytest.raises(ValueError):
            re.set(bad)
    assert re.set([(28, 36, 4, 4), (0, 0, 31, 39)]) == [(28, 36, 4, 4), (0, 0, 31, 39)]      # touching the corner is fine
    with pytest.raises(RuntimeError):
        _re(0.5).sample()                                                  # not bound: no image size to draw for
    with pytest.raises(RuntimeError):
        _re(0.5).set([None])


def test_state_dict_round_trips():
    a = _re(1.0, mode="pixel", seed=3).bind((4, 3, 32, 40))
    for _ in range(5):
        a.sample(rng=random.Random(1))
    sd = a.state_dict()
    assert sd == {"seed": 3, "counter": 5}
    b = _re(1.0, mode="pixel", seed=0).bind((4, 3, 32, 40))
    b.load_state_dict(sd)
    assert b.key() == a.key()
    assert a.sample(rng=random.Random(2)) == b.sample(rng=random.Random(2)) and a.packed() == b.packed()


def test_refusals():
    with pytest.raises(NotImplementedError):
        _re(0.25, mode="rand")
    for kw in ({"max_count": 2}, {"min_count": 2}, {"min_count": 2, "max_count": 3}, {"min_count": 0, "max_count": 1}):
        with pytest.raises(NotImplementedError):
            _re(0.25, mode="pixel", **kw)
    with pytest.raises(ValueError):
        _re(0.25, mode="colour")
    assert _re(0.25, mode="pixel", max_count=1).mode == "pixel" and _re(0.25).mode == "const"
    # erase= with hcs= is refused before anything touches a device
    from fastvim_amd.pipeline import SegmentedTrainStep
    with pytest.raises(ValueError, match="erase= and hcs="):
        SegmentedTrainStep(None, None, None, None, None, None, hcs=object(), erase=_re(0.25))
