"""Hierarchical channel sampling (HCS) of the channel models on the HIP path.

Every channel-model recipe of the reference trains with it (``hcs: True, channels: 8, sort_channels: True``): each training
forward of ``PatchEmbedPerChannel`` draws a channel COUNT ``c`` in 1..n and a SUBSET of ``c`` channels with Python's
``random`` (models/channel_wise_tokenization/models_channel_mamba_faster.py:170-175), slices the image and the channel
embedding with them, and runs the backbone with ``tokens_per_patch = c``.  Drawn inside ``forward`` and applied by
indexing, the subset is baked into a captured training step.  Here the host draws the same numbers in the same order
(``ChannelSampler.sample``) and writes the INDICES to an int32 array in device memory; the embedding kernels
(``fv_patch_unfold_chan``, ``fv_chan_embed_table``, ``fv_chan_embed_scatter``) read them when they RUN, so a replayed graph
embeds whatever subset the array holds at that moment -- the technique of ``Mixup``'s parameter block.  The COUNT fixes every
shape downstream and stays a host integer: ``SegmentedTrainStep(..., hcs=sampler)`` keeps one family of graphs per count and
replays the family of ``sampler.count``.

    x.copy_(batch); target.copy_(y); sampler.sample(); opt.set_lr(lr); step.step()
"""
import random

import torch

from ._devblock import BlockWriter


def draw(num_channels, sort_channels=True):
    """The reference's draw (:170-175), consuming Python's ``random`` exactly as it does: ``randint(1, n)``, then
    ``random.sample(range(n), k)``, sorted when ``sort_channels is True``.  The one place the draw is written down."""
    c_new = random.randint(1, num_channels)
    channels = random.sample(range(num_channels), k=c_new)
    if sort_channels is True:
        channels.sort()
    return channels


def check_subset(channels, num_channels):
    channels = [int(c) for c in channels]
    if not channels:
        raise ValueError("channel subset: empty")
    if min(channels) < 0 or max(channels) >= num_channels:
        raise ValueError(f"channel subset {channels}: indices must lie in [0, {num_channels})")
    if len(set(channels)) != len(channels):
        raise ValueError(f"channel subset {channels}: duplicate index")
    return channels


_writers = {}          # device index -> BlockWriter of ``upload``


def upload(channels, device):
    """A fresh int32 device array holding ``channels``: what a forward without a sampler hands its kernels (the array is
    the forward's own, so its backward may run any time later).  Outside a capture an asynchronous copy through a pinned
    staging ring; under stream capture -- where the values are frozen into the graph anyway -- element fills, which need
    no host memory at replay."""
    device = torch.device(device)
    sel = torch.empty(len(channels), device=device, dtype=torch.int32)
    if torch.cuda.is_current_stream_capturing():
        for k, c in enumerate(channels):
            sel[k:k + 1].fill_(int(c))
        return sel
    key = device.index if device.index is not None else torch.cuda.current_device()
    w = _writers.get(key)
    if w is None or w.n < len(channels):
        w = _writers[key] = BlockWriter(max(64, len(channels)), slots=8)
    w.write(sel, channels)
    return sel


class ChannelSampler:
    """The host-side draw of hierarchical channel sampling and the device array the embedding kernels read.

    ``sample()`` draws the next step's subset, ``set(channels)`` forces one (tests, resumed runs); both write the indices to
    the device array once it exists (``block(device)``; like ``Mixup``, nothing is written without a GPU).  ``count`` is the
    number of selected channels -- a host integer, because it fixes shapes; ``last()`` the current selection.  A new
    sampler selects every channel."""

    def __init__(self, num_channels, sort_channels=True):
        self.num_channels = int(num_channels)
        if self.num_channels < 1:
            raise ValueError("ChannelSampler: num_channels must be at least 1")
        self.sort_channels = sort_channels
        self._channels = list(range(self.num_channels))
        self._block = None                   # the device array, made on first need
        self._writer = None

    def sample(self):
        """Draw with Python's ``random`` in the reference's order (same ``random.seed``, same stream of subsets), write the
        indices to the device array and return the list."""
        self._channels = draw(self.num_channels, self.sort_channels)
        self._write()
        return list(self._channels)

    def set(self, channels):
        """Force the subset: distinct indices in [0, num_channels), at least one, in the order given."""
        self._channels = check_subset(channels, self.num_channels)
        self._write()
        return list(self._channels)

    def last(self):
        return list(self._channels)

    @property
    def count(self):
        return len(self._channels)

    def block(self, device=None):
        """The device array (``num_channels`` x int32; the first ``count`` entries are the selection), created on first use
        and rewritten by every ``sample()`` / ``set()`` from then on."""
        if self._block is None:
            device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            if device.type != "cuda":
                raise RuntimeError("fastvim_amd ops run on the GPU only (HIP kernels); the channel-index array needs a GPU device")
            self._block = torch.zeros(self.num_channels, device=device, dtype=torch.int32)
            self._writer = BlockWriter(self.num_channels)
            self._write()
        elif device is not None and torch.device(device).type == "cuda" and torch.device(device).index not in (None, self._block.device.index):
            raise RuntimeError(f"ChannelSampler: the index array lives on {self._block.device}, the tensors on {device}")
        return self._block

    def _write(self):
        if self._block is None:
            return
        # the entries behind the selection are filled with the channels left out: the array always holds a permutation
        rest = [c for c in range(self.num_channels) if c not in self._channels]
        self._writer.write(self._block, self._channels + rest)
