"""Batch-mode Mixup / CutMix on the HIP path: a drop-in for ``timm.data.Mixup`` as the reference trainer uses it
(``imgs, labels = self.mixup_fn(imgs, labels)``, imagenet_classification/supervised_imagenet.py:116-139; ``mixup: 0.8,
cutmix: 1.0, mixup_mode: 'batch', label_smoothing: 0.1`` in every ImageNet and MAE fine-tune config).

timm draws ``lam`` and the CutMix box with numpy on the host and bakes them into its kernels as Python scalars and slice
bounds, so a captured training step would replay the first batch's augmentation forever.  Here the host draws the same
numbers in the same order (``sample``) and writes them into a 32-byte MIX-PARAMETER BLOCK in device memory
(``struct fv_mix_params``, include/fastvim_hip.h); every kernel reads the block when it RUNS, so a replayed graph mixes
with whatever the block holds at that moment -- the way ``FlatAdamW.set_lr`` feeds the optimizer graph its learning rate.

Two ways to use it:

* drop-in, eager: ``x_mixed, target = mix(x, labels)`` -- ``sample()``, then ONE launch that mixes image b with image
  B-1-b (the batch read once, written once) and one that writes the dense (B, C) soft target.
* inside ``SegmentedTrainStep(..., mix.criterion(), x, labels, mixup=mix)``: the mixing happens inside the patch unfold
  (``fv_patch_unfold_mix``: the mixed batch never exists in memory) and the soft target inside the loss kernel
  (``fv_label_ce``: no (B, C) target tensor); the caller calls ``mix.sample()`` between steps.
"""
import collections
import struct

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from ._devblock import BlockWriter

MixParams = collections.namedtuple("MixParams", "lam use_cutmix box")      # box = (yl, yh, xl, xh) in pixels


def _hw(shape):
    if torch.is_tensor(shape):
        shape = shape.shape
    shape = tuple(int(v) for v in shape)
    if len(shape) < 2:
        raise ValueError(f"Mixup: an image shape ends in (H, W), got {shape}")
    return shape[-2], shape[-1]


class Mixup:
    """``timm.data.Mixup``'s constructor arguments; only ``mode='batch'`` without ``cutmix_minmax`` is built (no reference
    config uses anything else)."""

    def __init__(self, mixup_alpha=1., cutmix_alpha=0., cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='batch',
                 correct_lam=True, label_smoothing=0.1, num_classes=1000):
        if cutmix_minmax is not None:
            raise NotImplementedError("fastvim_amd.mixup.Mixup: cutmix_minmax is not implemented (no reference config sets it)")
        if mode != 'batch':
            raise NotImplementedError(f"fastvim_amd.mixup.Mixup: mode={mode!r} is not implemented, only 'batch' "
                                      "(what every reference config uses)")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.mix_prob, self.switch_prob = float(prob), float(switch_prob)
        self.mode, self.correct_lam = mode, bool(correct_lam)
        self.label_smoothing, self.num_classes = float(label_smoothing), int(num_classes)
        if not 0.0 <= self.label_smoothing < 1.0:
            raise ValueError("Mixup: label_smoothing must be in [0, 1)")
        self.mixup_enabled = True
        self._hw = None                      # image size the CutMix box is drawn for
        self._params = MixParams(1.0, False, (0, 0, 0, 0))
        self._block = None                   # the device block, made on first need
        self._writer = None                  # its BlockWriter (pinned staging ring), made with it

    # ------------------------------------------------------------------ host side
    def bind(self, x):
        """Remember the image size (a tensor or a shape ending in (H, W)) that ``sample()`` draws CutMix boxes for, and, for
        a GPU tensor, put the block on its device."""
        self._hw = _hw(x)
        if torch.is_tensor(x) and x.is_cuda:
            self.block(x.device)
        return self

    def sample(self, img_shape=None):
        """Draw the next batch's parameters with ``numpy.random`` in timm's order (same ``np.random.seed``, same stream of
        augmentations) and write them to the device block.  torch's generators are not touched.  Returns ``last()``."""
        if img_shape is not None:
            self._hw = _hw(img_shape)
        lam, use_cutmix, box = 1.0, False, (0, 0, 0, 0)
        if self.mixup_enabled and np.random.rand() < self.mix_prob:
            if self.mixup_alpha > 0. and self.cutmix_alpha > 0.:
                use_cutmix = bool(np.random.rand() < self.switch_prob)
                lam = np.random.beta(self.cutmix_alpha, self.cutmix_alpha) if use_cutmix else \
                    np.random.beta(self.mixup_alpha, self.mixup_alpha)
            elif self.mixup_alpha > 0.:
                lam = np.random.beta(self.mixup_alpha, self.mixup_alpha)
            elif self.cutmix_alpha > 0.:
                use_cutmix = True
                lam = np.random.beta(self.cutmix_alpha, self.cutmix_alpha)
            lam = float(lam)                 # (neither alpha > 0: nothing to mix, lam stays 1)
        if lam == 1.0:
            use_cutmix = False
        elif use_cutmix:
            if self._hw is None:
                raise RuntimeError("Mixup.sample(): a CutMix box needs the image size -- pass img_shape=, or call bind(x) / "
                                   "the object itself once")
            H, W = self._hw
            ratio = np.sqrt(1 - lam)
            cut_h, cut_w = int(H * ratio), int(W * ratio)
            cy = np.random.randint(0, H)
            cx = np.random.randint(0, W)
            yl, yh = int(np.clip(cy - cut_h // 2, 0, H)), int(np.clip(cy + cut_h // 2, 0, H))
            xl, xh = int(np.clip(cx - cut_w // 2, 0, W)), int(np.clip(cx + cut_w // 2, 0, W))
            box = (yl, yh, xl, xh)
            if self.correct_lam:
                lam = 1. - (yh - yl) * (xh - xl) / float(H * W)
        self._params = MixParams(lam, use_cutmix, box)
        self._write()
        return self._params

    def set(self, lam, use_cutmix=False, box=None):
        """Force the parameters (tests, resumed runs).  ``box = (yl, yh, xl, xh)``, required with ``use_cutmix``; ``lam`` then
        only weighs the labels (timm's ``correct_lam`` is the caller's business here)."""
        lam = float(lam)
        if not 0.0 <= lam <= 1.0:
            raise ValueError(f"Mixup.set: lam = {lam} is not in [0, 1]")
        if use_cutmix:
            if box is None or len(box) != 4:
                raise ValueError("Mixup.set: use_cutmix needs box=(yl, yh, xl, xh)")
            box = tuple(int(v) for v in box)
            if min(box) < 0 or box[0] > box[1] or box[2] > box[3]:
                raise ValueError(f"Mixup.set: bad box {box}")
        else:
            box = (0, 0, 0, 0)
        self._params = MixParams(lam, bool(use_cutmix), box)
        self._write()
        return self._params

    def last(self):
        """``MixParams(lam, use_cutmix, box)`` of the last ``sample()`` / ``set()``."""
        return self._params

    def packed(self):
        """The 32 bytes of ``struct fv_mix_params`` for the current parameters: ``lam`` and ``one_minus_lam`` as fp32 -- the
        latter the rounding of the DOUBLE ``1. - lam``, as torch receives Python's ``1. - lam``."""
        lam, cut, (yl, yh, xl, xh) = self._params
        return struct.pack("<ffiiiiii", lam, 1. - lam, int(cut), yl, yh, xl, xh, 0)

    # ------------------------------------------------------------------ device side
    def block(self, device=None):
        """The device mix-parameter block (8 x int32 storage), created on first use and rewritten by every ``sample()`` /
        ``set()`` from then on."""
        if self._block is None:
            device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            if device.type != "cuda":
                raise RuntimeError("fastvim_amd ops run on the GPU only (HIP kernels); the mix-parameter block needs a GPU device")
            self._block = torch.zeros(8, device=device, dtype=torch.int32)
            self._writer = BlockWriter(8)
            self._write()
        elif device is not None and torch.device(device).type == "cuda" and torch.device(device).index not in (None, self._block.device.index):
            raise RuntimeError(f"Mixup: the parameter block lives on {self._block.device}, the tensors on {device}")
        return self._block

    def _write(self):
        if self._block is None:
            return
        # an asynchronous copy from pinned memory on the current stream, no host wait (fastvim_amd/_devblock.py)
        self._writer.write(self._block, self.packed())

    def _check_batch(self, x):
        if x.shape[0] % 2 != 0:
            raise ValueError(f"Mixup: batch mode pairs sample b with sample B-1-b, the batch size ({x.shape[0]}) must be even")

    def mix_batch(self, x, out=None):
        """``out[b] = mix(x[b], x[B-1-b])`` with the block's current parameters (no draw); ``x`` is left untouched."""
        from .glue_ops import mix_batch
        self._check_batch(x)
        L.require_gpu(x)
        return mix_batch(x, self.block(x.device), out=out)

    def target(self, labels):
        """The dense (B, C) fp32 soft target timm returns for ``labels`` (B,) int64 under the current parameters."""
        self._check_batch(labels)
        L.require_gpu(labels)
        if labels.dim() != 1 or labels.dtype != torch.int64:
            raise RuntimeError(f"Mixup: labels must be (B,) int64 class indices, got {tuple(labels.shape)} {labels.dtype}")
        lab = labels.contiguous()
        B = lab.shape[0]
        out = torch.empty(B, self.num_classes, device=lab.device, dtype=torch.float32)
        import ctypes
        rc = L.lib().fv_mixup_target(L.ptr(lab), L.ptr(out), L.i32(B), L.i32(self.num_classes), ctypes.c_double(self.label_smoothing),
                                     L.ptr(self.block(lab.device)), L.stream_of(lab))
        L.check(rc, "mixup_target")
        return out

    def __call__(self, x, target):
        """``(x_mixed, soft_target)`` like timm's; unlike timm's, ``x`` is not modified (the reference only uses the return
        value)."""
        self._check_batch(x)
        L.require_gpu(x, target)
        self.bind(x)
        self.sample()
        return self.mix_batch(x), self.target(target)

    def criterion(self):
        """The loss that goes with this augmentation inside a captured step: ``forward(logits, labels)`` with the (B,) int64
        labels of the UNMIXED batch; the soft target is built inside the loss kernel from labels[b], labels[B-1-b] and this
        object's block."""
        return MixupCrossEntropy(self)


class MixupCrossEntropy(nn.Module):
    """``SoftTargetCrossEntropy()(logits, mix.target(labels))`` bit for bit, without the target tensor: one ``fv_label_ce``
    launch for value and gradient."""

    def __init__(self, mixup):
        super().__init__()
        self.mixup = mixup

    def forward(self, logits, labels):
        from .losses import _LabelCEFn
        m = self.mixup
        if logits.shape[-1] != m.num_classes:
            raise RuntimeError(f"MixupCrossEntropy: logits have {logits.shape[-1]} classes, the Mixup was built for {m.num_classes}")
        m._check_batch(logits)
        L.require_gpu(logits, labels)
        return _LabelCEFn.apply(logits, labels, m.block(logits.device), m.label_smoothing)
