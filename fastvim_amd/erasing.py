"""Random erasing on the HIP path: a drop-in for ``timm.data.random_erasing.RandomErasing`` as the reference's loaders use it
(``re_prob: 0.25, re_mode: 'pixel', re_count: 1`` in every ImageNet and MAE fine-tune config; per sample, after ``ToTensor``
and ``Normalize``, before the batch-level Mixup of ``training_step``: imagenet_classification/datasets_supervised.py,
mae/datasets_finetune.py).

Erasing acts on the NORMALISED float image, so it is the one loader stage that cannot be done before a uint8 batch
(fastvim_amd/pixels.py) leaves the host.  Here the host only draws the BOXES -- with Python's ``random`` in timm's order, so
the same ``random.seed`` gives the same boxes -- and writes them, with a mode and a 64-bit noise key, into an ERASE BLOCK in
device memory (include/fastvim_hip.h, at ``fv_random_erase``): ``4 + 4 * B`` int32, ``key0, key1, mode, B``, then ``top,
left, h, w`` per sample, ``h == 0`` meaning no erase.  The kernels read the block when they RUN, so a replayed graph
erases with the values of the last ``sample()`` -- the technique of ``Mixup``'s parameter block.  The pixels are replaced on
the device: by 0 (``mode='const'``), or by a standard-normal value per (channel, y, x) that is a pure function of (key, b,
c, y, x) (Philox4x32-10 + Box-Muller, csrc/erase_noise.h) -- the same bits from every kernel.

Where timm fills a box with ``torch.empty(...).normal_()`` from torch's generator, the noise here comes from the key: the
BOXES reproduce a timm run draw for draw, the noise values are an independent standard-normal stream.  The key is derived
on the host from ``(seed, counter)``; the counter advances once per ``sample()``.  Data-parallel ranks must pass DIFFERENT
seeds (``seed=rank``): sample b of every rank would otherwise get the same noise at the same position.  torch's and
numpy's generators are never touched.

Three ways to use it:

* eager: ``x_erased = re(x_float)`` -- ``bind``, ``sample()``, one ``fv_random_erase`` launch, out of place.
* inside ``SegmentedTrainStep(..., x_u8, labels, mixup=mix, erase=re)``: the pixels are replaced inside the uint8 patch
  unfold, between the table lookup and the mixing (``fv_patch_unfold_u8_re`` / ``fv_patch_unfold_mix_u8_re``: each image of
  a Mixup pair with its own box first, mixed afterwards).  The caller calls ``re.sample()`` between steps.
* with a float ``x`` the step runs ``fv_random_erase`` out of place into a scratch batch in front of the embedding.
"""
import math
import random
import struct

import torch

from . import _lib as L
from ._devblock import BlockWriter

MODES = {"const": 0, "pixel": 1}          # FV_ERASE_CONST, FV_ERASE_PIXEL
_M64 = (1 << 64) - 1


def _splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def derive_key(seed, counter):
    """``(key0, key1)``, two 32-bit words, from the 64-bit ``seed`` and draw ``counter``: the low and the high half of
    ``splitmix64(splitmix64(seed) ^ counter)`` -- neighbouring seeds and neighbouring counters give unrelated keys."""
    k = _splitmix64(_splitmix64(int(seed) & _M64) ^ (int(counter) & _M64))
    return k & 0xffffffff, k >> 32


def _bchw(x):
    shape = tuple(int(v) for v in (x.shape if torch.is_tensor(x) else x))
    if len(shape) != 4:
        raise ValueError(f"RandomErasing: expected a (B, C, H, W) batch or shape, got {shape}")
    return shape


class RandomErasing:
    """``timm.data.random_erasing.RandomErasing``'s constructor arguments plus ``seed``.  Only ``mode='const'`` and
    ``mode='pixel'`` with exactly one box per sample are built (what every reference config uses): ``mode='rand'`` and
    any count other than 1 raise ``NotImplementedError``."""

    def __init__(self, probability=0.5, min_area=0.02, max_area=1 / 3, min_aspect=0.3, max_aspect=None, mode='const',
                 min_count=1, max_count=None, seed=0):
        mode = mode.lower()
        if mode == 'rand':
            raise NotImplementedError("fastvim_amd.erasing.RandomErasing: mode='rand' (one colour per box) is not implemented, "
                                      "only 'const' and 'pixel' (no reference config uses it)")
        if mode not in MODES:
            raise ValueError(f"RandomErasing: mode must be 'const' or 'pixel', got {mode!r}")
        max_count = max_count or min_count
        if min_count != 1 or max_count != 1:
            raise NotImplementedError(f"fastvim_amd.erasing.RandomErasing: min_count={min_count}, max_count={max_count} is not "
                                      "implemented, only one box per sample (what every reference config uses)")
        max_aspect = max_aspect or 1 / min_aspect
        self.probability, self.min_area, self.max_area = float(probability), float(min_area), float(max_area)
        self.log_aspect_ratio = (math.log(min_aspect), math.log(max_aspect))
        self.mode, self.min_count, self.max_count = mode, 1, 1
        self.seed, self.counter = int(seed) & _M64, 0
        self._shape = None                   # (B, H, W) the boxes are drawn for
        self._boxes = []                     # (top, left, h, w) per sample; h == 0: no erase
        self._block = None                   # the device block, made on first need
        self._writer = None

    # ------------------------------------------------------------------ host side
    def bind(self, x):
        """Remember the batch size and the image size (a tensor or a (B, C, H, W) shape) that ``sample()`` draws for -- until
        the first ``sample()`` / ``set()`` no sample has a box -- and, for a GPU tensor, put the block on its device.  The
        block is sized by the batch: once it exists the batch size is fixed (captured launches hold its address)."""
        B, _, H, W = _bchw(x)
        if self._block is not None and self._shape is not None and self._shape[0] != B:
            raise RuntimeError(f"RandomErasing: the device block was made for batches of {self._shape[0]}, got {B}")
        if self._shape != (B, H, W):
            self._shape = (B, H, W)
            self._boxes = [(0, 0, 0, 0)] * B
            self._write()
        if torch.is_tensor(x) and x.is_cuda:
            self.block(x.device)
        return self

    def _bound(self, what):
        if self._shape is None:
            raise RuntimeError(f"RandomErasing.{what}: the batch and image size are unknown -- call bind(x) (or the object "
                               "itself) first")
        return self._shape

    def sample(self, rng=None):
        """Draw the next batch's boxes, sample 0 to B-1, with Python's ``random`` (or ``rng``, a ``random.Random``) exactly as
        timm's ``_erase`` consumes it: ``random() > probability`` -> no box; else up to 10 attempts of ``uniform(min_area,
        max_area) * (H * W)``, ``exp(uniform(log min_aspect, log max_aspect))``, ``h = int(round(sqrt(area * ar)))``, ``w =
        int(round(sqrt(area / ar)))``, accepted if ``w < W and h < H`` with ``top = randint(0, H - h)``, ``left = randint(0,
        W - w)``.  Then the draw counter advances (a new noise key) and the block is written.  Returns ``last()``."""
        B, H, W = self._bound("sample()")
        r = random if rng is None else rng
        area = H * W
        boxes = []
        for _ in range(B):
            box = (0, 0, 0, 0)
            if not r.random() > self.probability:
                for _attempt in range(10):
                    target_area = r.uniform(self.min_area, self.max_area) * area / 1      # (timm: / count)
                    aspect_ratio = math.exp(r.uniform(*self.log_aspect_ratio))
                    h = int(round(math.sqrt(target_area * aspect_ratio)))
                    w = int(round(math.sqrt(target_area / aspect_ratio)))
                    if w < W and h < H:
                        top = r.randint(0, H - h)
                        left = r.randint(0, W - w)
                        box = (top, left, h, w) if h > 0 and w > 0 else (0, 0, 0, 0)      # (an empty slice erases nothing)
                        break
            boxes.append(box)
        self._boxes = boxes
        self.counter = (self.counter + 1) & _M64
        self._write()
        return self.last()

    def set(self, boxes):
        """Force the boxes (tests, resumed runs): one entry per sample, ``None`` or ``(top, left, h, w)`` with the box inside
        the image; ``h == 0`` or ``None``: no erase.  The counter -- the noise key -- stays."""
        B, H, W = self._bound("set()")
        boxes = list(boxes)
        if len(boxes) != B:
            raise ValueError(f"RandomErasing.set: {len(boxes)} boxes for a batch of {B}")
        out = []
        for b, box in enumerate(boxes):
            if box is None:
                out.append((0, 0, 0, 0))
                continue
            if len(box) != 4:
                raise ValueError(f"RandomErasing.set: box {b} must be (top, left, h, w), got {box!r}")
            top, left, h, w = (int(v) for v in box)
            if h == 0 or w == 0:
                out.append((0, 0, 0, 0))
                continue
            if min(top, left, h, w) < 0 or top + h > H or left + w > W:
                raise ValueError(f"RandomErasing.set: box {b} = {(top, left, h, w)} does not lie inside the {H}x{W} image")
            out.append((top, left, h, w))
        self._boxes = out
        self._write()
        return self.last()

    def last(self):
        """The ``(top, left, h, w)`` of every sample from the last ``sample()`` / ``set()``; ``(0, 0, 0, 0)``: not erased."""
        return list(self._boxes)

    def key(self):
        """``(key0, key1)`` of the current ``(seed, counter)``."""
        return derive_key(self.seed, self.counter)

    def packed(self):
        """The ``16 + 16 * B`` bytes of the erase block for the current state."""
        k0, k1 = self.key()
        flat = [v for box in self._boxes for v in box]
        return struct.pack(f"<IIii{len(flat)}i", k0, k1, MODES[self.mode], len(self._boxes), *flat)

    def state_dict(self):
        return {"seed": self.seed, "counter": self.counter}

    def load_state_dict(self, state):
        self.seed, self.counter = int(state["seed"]) & _M64, int(state["counter"]) & _M64
        self._write()

    # ------------------------------------------------------------------ device side
    def block(self, device=None):
        """The device erase block (``4 + 4 * B`` int32), created on first use and rewritten by every ``sample()`` / ``set()``
        from then on."""
        if self._block is None:
            B = self._bound("block()")[0]
            device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            if device.type != "cuda":
                raise RuntimeError("fastvim_amd ops run on the GPU only (HIP kernels); the erase block needs a GPU device")
            self._block = torch.zeros(4 + 4 * B, device=device, dtype=torch.int32)
            self._writer = BlockWriter(4 + 4 * B)
            self._write()
        elif device is not None and torch.device(device).type == "cuda" and torch.device(device).index not in (None, self._block.device.index):
            raise RuntimeError(f"RandomErasing: the erase block lives on {self._block.device}, the tensors on {device}")
        return self._block

    def _write(self):
        if self._block is None:
            return
        # an asynchronous copy from pinned memory on the current stream, no host wait (fastvim_amd/_devblock.py)
        self._writer.write(self._block, self.packed())

    def _check_batch(self, x):
        B, _, H, W = _bchw(x)
        if self._shape != (B, H, W):
            raise ValueError(f"RandomErasing: bound to batches of {self._shape} (B, H, W), got {(B, H, W)}")

    def erase(self, x, out=None):
        """``x`` (B, C, H, W) fp32 or bf16 with the current boxes and key applied (no draw), out of place unless ``out is x``."""
        from .glue_ops import random_erase
        L.require_gpu(x)
        self._check_batch(x)
        return random_erase(x, self.block(x.device), out=out)

    def __call__(self, x):
        """The eager form on a normalised float batch: draw, then erase.  Unlike timm's, ``x`` is not modified."""
        L.require_gpu(x)
        self.bind(x)
        self.sample()
        return self.erase(x)
