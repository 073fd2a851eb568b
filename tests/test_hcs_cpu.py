"""Host side of hierarchical channel sampling (fastvim_amd/hcs.py): ``ChannelSampler`` draws what the reference's
``PatchEmbedPerChannel.forward`` draws (models_channel_mamba_faster.py:170-175), consuming Python's ``random`` in the same
order.  No GPU needed: without one the device array is simply not made (the rule of ``Mixup``)."""
import random

import pytest

from conftest import load_golden
from fastvim_amd.hcs import ChannelSampler


def _reference_draw(n, sort_channels):
    """:170-175, restated."""
    c_new = random.randint(1, n)
    channels = random.sample(range(n), k=c_new)
    if sort_channels is True:
        channels.sort()
    return channels


def test_sampler_draws_the_golden_subset():
    c = load_golden("channel.pt")["tiny_64x96_c5_hcs"]
    random.seed(c["py_seed"])
    s = ChannelSampler(c["channels"])
    assert c["py_seed"] == 1234 and c["channels"] == 5
    assert s.sample() == c["subset"] == [0, 2, 3, 4]
    assert s.last() == c["subset"] and s.count == 4


@pytest.mark.parametrize("seed", [0, 2, 1234, 99991])
@pytest.mark.parametrize("sort_channels", [True, False])
def test_sampler_consumes_random_like_the_reference(seed, sort_channels):
    n, steps = 8, 40
    random.seed(seed)
    want = []
    for _ in range(steps):
        ch = _reference_draw(n, sort_channels)
        want.append((ch, random.getstate()))
    random.seed(seed)
    s = ChannelSampler(n, sort_channels=sort_channels)
    for ch, state in want:
        got = s.sample()
        assert got == ch and s.last() == ch and s.count == len(ch)
        assert random.getstate() == state
        assert 1 <= s.count <= n and len(set(got)) == len(got) and all(0 <= v < n for v in got)
    if sort_channels:
        assert all(ch == sorted(ch) for ch, _ in want)
    else:
        assert any(ch != sorted(ch) for ch, _ in want)          # the drawn order is kept


def test_new_sampler_selects_every_channel():
    s = ChannelSampler(6)
    assert s.last() == [0, 1, 2, 3, 4, 5] and s.count == 6 and s.num_channels == 6
    with pytest.raises(ValueError):
        ChannelSampler(0)


def test_set_validates():
    s = ChannelSampler(8)
    state = random.getstate()
    assert s.set([6, 1, 3]) == [6, 1, 3] and s.last() == [6, 1, 3] and s.count == 3          # the order given is kept
    assert s.set(range(8)) == list(range(8))
    for bad in ([], [8], [-1, 2], [0, 3, 3], [1, 2, 9]):
        with pytest.raises(ValueError):
            s.set(bad)
    assert s.last() == list(range(8))                            # a refused subset changes nothing
    assert random.getstate() == state                            # set() draws nothing
    lst = s.last()
    lst.append(99)
    assert s.last() == list(range(8))                            # last() hands out a copy


def test_sample_without_a_gpu_leaves_the_block_unmade():
    s = ChannelSampler(8)
    s.sample()
    s.set([2, 5])
    assert s._block is None
    with pytest.raises(RuntimeError):
        s.block("cpu")


def test_mixup_and_sampler_share_one_block_writer():
    """The pinned-ring writer lives in one place (fastvim_amd/_devblock.py); neither class carries a copy."""
    import inspect
    from fastvim_amd import _devblock, hcs, mixup
    assert mixup.BlockWriter is _devblock.BlockWriter and hcs.BlockWriter is _devblock.BlockWriter
    for mod in (mixup, hcs):
        assert "pin_memory" not in inspect.getsource(mod)
