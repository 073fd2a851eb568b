"""Training losses of the reference recipe on the HIP path.

``SoftTargetCrossEntropy`` is a drop-in for ``timm.loss.SoftTargetCrossEntropy`` as the reference trainer uses it under
mixup / label smoothing (imagenet_classification/supervised_imagenet.py:83, 109-115):
``loss = mean_b sum_c -target[b, c] * log_softmax(x[b])[c]``.  Value and gradient come from ONE fused launch
(csrc/loss.hip, C ABI ``fv_soft_target_ce``) instead of the eleven small kernels of the eager expression and its
autograd.  ``target`` is treated as a constant (no gradient), as in the reference's use.

``CrossEntropyLoss`` and ``LabelSmoothingCrossEntropy`` are the trainer's other two branches (:80-92) and the loss of every
``validation_step``: integer labels, mean reduction.  They run on ``fv_label_ce``, which is the same row kernel with the
target built in registers from the label instead of read from a (B, C) tensor; ``fastvim_amd.mixup.Mixup.criterion()``
is that kernel once more, with the partner label and the mixing weights of a batch-mode Mixup / CutMix.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib as L


class _SoftTargetCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, target):
        L.require_gpu(x, target)
        if x.dim() != 2 or target.shape != x.shape:
            raise RuntimeError(f"SoftTargetCrossEntropy: logits {tuple(x.shape)} and target {tuple(target.shape)} must be (B, C)")
        B, C = x.shape
        xc = x.contiguous()
        if xc.dtype not in (torch.float32, torch.bfloat16):
            xc = xc.float()
        t = target.detach().float().contiguous()
        rows = torch.empty(B, device=x.device, dtype=torch.float32)
        loss = torch.empty(1, device=x.device, dtype=torch.float32)
        dx = torch.empty(B, C, device=x.device, dtype=torch.float32)
        rc = L.lib().fv_soft_target_ce(L.ptr(xc), L.i32(L.dtype_code(xc.dtype)), L.ptr(t), L.ptr(rows), L.ptr(loss), L.ptr(dx),
                                       L.i32(B), L.i32(C), L.stream_of(xc))
        L.check(rc, "soft_target_ce")
        ctx.save_for_backward(dx)
        ctx.x_dtype = x.dtype
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        if ctx.x_dtype in (torch.float32, torch.bfloat16) and g.dtype == torch.float32 and g.numel() == 1:
            from .glue_ops import scale_cast
            return scale_cast(dx, g, ctx.x_dtype), None           # scale by the upstream scalar and cast, one launch
        return (dx * g).to(ctx.x_dtype), None


class SoftTargetCrossEntropy(nn.Module):
    """``forward(x, target)``: x (B, C) logits (fp32 or bf16), target (B, C) soft labels -> scalar fp32 loss."""

    def forward(self, x, target):
        return _SoftTargetCEFn.apply(x, target)


def _label_ce(x, labels, block, smoothing, want_grad, want_correct):
    """One ``fv_label_ce`` call -> (loss (1,), dlogits or None, (correct_rows, n_correct) or None)."""
    L.require_gpu(x, labels, block)
    if x.dim() != 2 or labels.shape != x.shape[:1]:
        raise RuntimeError(f"label cross-entropy: logits {tuple(x.shape)} must be (B, C) and labels {tuple(labels.shape)} (B,)")
    if labels.dtype != torch.int64:
        raise RuntimeError(f"label cross-entropy: labels must be int64 class indices, got {labels.dtype}")
    B, C = x.shape
    xc = x.detach().contiguous()
    if xc.dtype not in (torch.float32, torch.bfloat16):
        xc = xc.float()
    lab = labels.contiguous()
    rows = torch.empty(B, device=x.device, dtype=torch.float32)
    loss = torch.empty(1, device=x.device, dtype=torch.float32)
    dx = torch.empty(B, C, device=x.device, dtype=torch.float32) if want_grad else None
    correct = (torch.empty(B, device=x.device, dtype=torch.int32), torch.empty(1, device=x.device, dtype=torch.int32)) if want_correct else None
    rc = L.lib().fv_label_ce(L.ptr(xc), L.i32(L.dtype_code(xc.dtype)), L.ptr(lab), L.ptr(block), ctypes.c_double(smoothing),
                             L.ptr(rows), L.ptr(loss), L.ptr(dx), L.ptr(correct[0] if correct else None),
                             L.ptr(correct[1] if correct else None), L.i32(B), L.i32(C), L.stream_of(xc))
    L.check(rc, "label_ce")
    return loss, dx, correct


class _LabelCEFn(torch.autograd.Function):
    """``block``: the device mix-parameter block of a ``Mixup`` (the target mixes labels[b] and labels[B-1-b] with the
    weights the block holds when the kernel RUNS), or None (the target is the smoothed one-hot of labels[b])."""

    @staticmethod
    def forward(ctx, x, labels, block, smoothing):
        loss, dx, _ = _label_ce(x, labels, block, smoothing, True, False)
        ctx.save_for_backward(dx)
        ctx.x_dtype = x.dtype
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        if ctx.x_dtype in (torch.float32, torch.bfloat16) and g.dtype == torch.float32 and g.numel() == 1:
            from .glue_ops import scale_cast
            return scale_cast(dx, g, ctx.x_dtype), None, None, None      # scale by the upstream scalar and cast, one launch
        return (dx * g).to(ctx.x_dtype), None, None, None


class LabelSmoothingCrossEntropy(nn.Module):
    """Drop-in for ``timm.loss.LabelSmoothingCrossEntropy``: ``mean_b (confidence * nll_b + smoothing * mean_c -logp[b, c])``,
    i.e. the soft-target loss on ``confidence * one_hot + smoothing / C``.  ``forward(x, labels)``: x (B, C) logits (fp32 or
    bf16, C <= 2048), labels (B,) int64 -> scalar fp32 loss; value and gradient from one launch."""

    def __init__(self, smoothing=0.1):
        super().__init__()
        assert 0.0 <= smoothing < 1.0
        self.smoothing = float(smoothing)
        self.confidence = 1.0 - self.smoothing

    def forward(self, x, target):
        return _LabelCEFn.apply(x, target, None, self.smoothing)

    def loss_and_correct(self, x, target):
        """Validation (supervised_imagenet.py:151-183): ``(loss, n_correct)`` -- the loss value without a gradient and the
        number of rows whose arg-max is the label (a 0-dim int32 device tensor), one launch."""
        loss, _, (_, n) = _label_ce(x, target, None, self.smoothing, False, True)
        return loss[0], n[0]


class CrossEntropyLoss(LabelSmoothingCrossEntropy):
    """Drop-in for ``torch.nn.CrossEntropyLoss()`` as the reference uses it: integer labels, mean reduction, no class
    weights, no ignore_index."""

    def __init__(self):
        super().__init__(smoothing=0.0)


def top1_correct(logits, labels):
    """(B,) bool: ``logits.argmax(1) == labels`` (the first maximum on a tie), from the loss kernel's arg-max pass."""
    _, _, (rows, _) = _label_ce(logits, labels, None, 0.0, False, True)
    return rows.bool()
