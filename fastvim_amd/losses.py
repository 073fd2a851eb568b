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


# ---------------------------------------------------------------------------------------------------------------------
# MAE reconstruction loss (csrc/mae_loss.hip, C ABI ``fv_mae_loss_fwd`` / ``fv_mae_loss_bwd``)
MAE_LOSS_MAX_PATCH = 28
MAE_LOSS_MAX_PATCHES = 128 * 1024


def mae_reconstruction_loss_ok(imgs, pred, mask, patch_size, table=None):
    """Whether ``mae_reconstruction_loss`` takes these tensors: the shape rule of the C predicate ``fv_mae_loss_ok`` (3
    channels, square images of whole patches, patch even in [8, 28], ``pred`` fp32 or bf16, at most 128 x 1024 patches) plus
    what only the host sees: GPU tensors on one device, NCHW-contiguous images (fp32, or uint8 with a (3, 256) fp32 table)
    that do not require grad, a contiguous ``pred`` (N, L, 3 p^2) and a contiguous fp32 ``mask`` (N, L).  Pure Python: no
    GPU and no library needed to ask."""
    p = int(patch_size)
    if imgs.dim() != 4 or pred.dim() != 3 or mask.dim() != 2:
        return False
    N, C, H, W = imgs.shape
    if N <= 0 or C != 3 or H <= 0 or H != W or p < 8 or p > MAE_LOSS_MAX_PATCH or p % 2 or H % p:
        return False
    Lp = (H // p) * (W // p)
    if N * Lp > MAE_LOSS_MAX_PATCHES or pred.dtype not in (torch.float32, torch.bfloat16):
        return False
    if tuple(pred.shape) != (N, Lp, 3 * p * p) or tuple(mask.shape) != (N, Lp) or mask.dtype != torch.float32:
        return False
    if not (imgs.is_cuda and pred.device == imgs.device and mask.device == imgs.device):
        return False
    if not (imgs.is_contiguous() and pred.is_contiguous() and mask.is_contiguous()):
        return False
    if imgs.requires_grad or mask.requires_grad:
        return False
    if table is None:
        return imgs.dtype == torch.float32
    return (imgs.dtype == torch.uint8 and table.dtype == torch.float32 and tuple(table.shape) == (3, 256)
            and table.is_contiguous() and table.device == imgs.device and table.data_ptr() % 16 == 0)


class _MAELossFn(torch.autograd.Function):
    """Differentiable in ``pred`` only.  Saves (mean, rstd) per patch and sum(mask) -- both stay on the device, nothing is
    synchronised: safe under graph capture -- and recomputes the target from the image in the backward launch."""

    @staticmethod
    def forward(ctx, pred, imgs, mask, table, patch, norm_pix):
        N, Lp, D = pred.shape
        dev = pred.device
        rows = torch.empty(N, Lp, device=dev, dtype=torch.float32)
        stats = torch.empty(N, Lp, 2, device=dev, dtype=torch.float32)
        out = torch.empty(2, device=dev, dtype=torch.float32)
        rc = L.lib().fv_mae_loss_fwd(L.ptr(imgs), L.ptr(table), L.ptr(pred), L.i32(L.dtype_code(pred.dtype)), L.ptr(mask),
                                     L.ptr(rows), L.ptr(stats), L.ptr(out), L.i32(N), L.i32(imgs.shape[2]), L.i32(imgs.shape[3]),
                                     L.i32(patch), L.i32(1 if norm_pix else 0), L.stream_of(pred))
        L.check(rc, "mae_loss_fwd")
        ctx.save_for_backward(pred, imgs, mask, table, stats, out)
        ctx.patch = patch
        ctx.mark_non_differentiable(rows, stats)
        return out[0], rows, stats

    @staticmethod
    def backward(ctx, g, _g_rows, _g_stats):
        pred, imgs, mask, table, stats, out = ctx.saved_tensors
        g = g.detach().to(device=pred.device, dtype=torch.float32).reshape(1).contiguous()
        dpred = torch.empty_like(pred)
        rc = L.lib().fv_mae_loss_bwd(L.ptr(imgs), L.ptr(table), L.ptr(pred), L.i32(L.dtype_code(pred.dtype)), L.ptr(mask),
                                     L.ptr(stats), L.ptr(out[1:]), L.ptr(g), L.ptr(dpred), L.i32(pred.shape[0]),
                                     L.i32(imgs.shape[2]), L.i32(imgs.shape[3]), L.i32(ctx.patch), L.stream_of(pred))
        L.check(rc, "mae_loss_bwd")
        return dpred, None, None, None, None, None


def mae_reconstruction_loss(imgs, pred, mask, patch_size, norm_pix_loss=True, table=None, return_rows=False):
    """The MAE loss of ``MaskedAutoencoderViM.forward_loss`` from two launches (and one backward): ``imgs`` (N, 3, H, W) fp32,
    or uint8 with ``table`` (the (3, 256) fp32 table of ``fastvim_amd.pixels``), ``pred`` (N, L, 3 p^2) fp32 or bf16 (inside
    ``torch.autocast`` it simply arrives as bf16; the arithmetic is fp32), ``mask`` (N, L) fp32 with 1 = removed.  Returns
    the scalar fp32 loss, differentiable in ``pred`` (the gradient has ``pred``'s dtype); with ``return_rows`` also
    ``loss_rows`` (N, L), the per-patch mean squared error (0 on kept patches), for logging.  The uint8 form equals the float
    form on ``pixels.lookup(table, imgs)`` bit for bit.  Raises where ``mae_reconstruction_loss_ok`` says no: the caller
    chooses the fallback."""
    if not mae_reconstruction_loss_ok(imgs, pred, mask, patch_size, table):
        raise RuntimeError(f"mae_reconstruction_loss: unsupported arguments (images {tuple(imgs.shape)} {imgs.dtype}, pred "
                           f"{tuple(pred.shape)} {pred.dtype}, mask {tuple(mask.shape)} {mask.dtype}, patch {patch_size}, "
                           f"table {'given' if table is not None else 'none'}); see mae_reconstruction_loss_ok")
    loss, rows, _ = _MAELossFn.apply(pred, imgs, mask, table, int(patch_size), bool(norm_pix_loss))
    return (loss, rows) if return_rows else loss
