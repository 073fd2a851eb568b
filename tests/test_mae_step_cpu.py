"""The MAE masking noise's restatement (tests/mask_noise_ref.py) and the host logic of ``MaskSampler``: no GPU."""
import numpy as np
import pytest
import torch

import mask_noise_ref as N


def test_restatement_is_in_the_unit_interval_and_exact_in_fp32():
    for seed, counter in ((0, 1), (2 ** 40 + 3, 2 ** 32 + 5)):
        v = N.noise_f64(seed, counter, 3, 197)
        assert v.shape == (3, 197) and float(v.min()) >= 0.0 and float(v.max()) < 1.0
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v)              # the fp32 cast loses nothing
        assert np.array_equal(v * 2.0 ** 24, np.floor(v * 2.0 ** 24))                  # the 2^-24 grid
        t = N.noise(seed, counter, 3, 197)
        assert t.dtype == torch.float32 and np.array_equal(t.double().numpy(), v)


def test_restatement_depends_on_seed_and_counter_and_sample():
    a = N.noise(0, 1, 2, 196)
    assert not torch.equal(a, N.noise(1, 1, 2, 196))
    assert not torch.equal(a, N.noise(0, 2, 2, 196))
    assert not torch.equal(a, N.noise(2 ** 32, 1, 2, 196))          # the high word of the seed is part of the key
    assert not torch.equal(a, N.noise(0, 2 ** 32 + 1, 2, 196))      # the high word of the counter is part of the counter
    assert not torch.equal(a[0], a[1])
    assert torch.equal(a, N.noise(0, 1, 2, 196))
    assert torch.equal(a[:, :15], N.noise(0, 1, 2, 15))             # a value depends on (b, l), not on the shape


def test_restatement_agrees_with_the_scalar_philox():
    for seed, counter in ((0, 1), (2 ** 40 + 3, 2 ** 32 + 5)):
        v = N.noise_f64(seed, counter, 3, 23)
        for b in range(3):
            for l in range(23):
                assert v[b, l] == N.noise_at(seed, counter, b, l), (seed, counter, b, l)


def test_tie_case_exists():
    """Seed 2, first ``sample()``, (8, 1024): sample 5 holds repeated values -- the case in which the plan's stable order
    (equal values ranked by token index) decides.  Asserted so that a change of the definition cannot silently lose it."""
    c = N.TIE_CASE
    v = N.noise_f64(c["seed"], c["counter"], c["B"], c["L"])
    row = v[c["sample"]]
    assert len(np.unique(row)) < row.size


def test_mask_sampler_host_logic():
    from fastvim_amd.mae_tokens import MaskSampler
    s = MaskSampler(seed=7)
    assert s.last() == (7, 0)
    for _ in range(5):
        s.sample()
    assert s.last() == (7, 5) and s.words() == (7, 0, 5, 0)
    sd = s.state_dict()
    assert sd == {"seed": 7, "counter": 5}
    t = MaskSampler(seed=0)
    t.load_state_dict(sd)
    assert t.last() == s.last() and t.words() == s.words()
    assert t.sample() == (7, 6)
    t.set_counter(2 ** 32 + 4)
    assert t.sample() == (7, 2 ** 32 + 5) and t.words() == (7, 0, 5, 1)
    big = MaskSampler(seed=2 ** 40 + 3)
    assert big.words()[:2] == (3, 2 ** 8) and big.words() == N.key_words(2 ** 40 + 3, 0)
    big.sample()
    assert big.words() == N.key_words(2 ** 40 + 3, 1)


def test_plan_shape_predicate():
    from fastvim_amd.mae_tokens import plan_shape_ok
    assert plan_shape_ok(128, (14, 14), 49) and plan_shape_ok(1, (32, 32), 1023) and plan_shape_ok(2, (3, 5), 3)
    assert not plan_shape_ok(2, (4, 4), 2)              # fewer than 3 kept
    assert not plan_shape_ok(2, (33, 32), 100)          # more than 1024 tokens
    assert not plan_shape_ok(2, (4, 4), 17) and not plan_shape_ok(0, (4, 4), 4)


def test_step_rejects_what_it_cannot_serve():
    """The construction checks that need no device: they come before anything touches the GPU."""
    from fastvim_amd.mae_step import MAEPretrainStep

    class Bare(torch.nn.Module):
        token_size = (4, 4)

    with pytest.raises(TypeError, match="_embed_masked"):
        MAEPretrainStep(Bare(), None, None, torch.zeros(2, 3, 64, 64), None)
