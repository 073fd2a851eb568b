"""Dense-prediction operators on the HIP kernels of csrc/chan_ln.hip: LayerNorm over C where one side is NCHW.

* ``tap_layer_norm_nchw(hidden, weight, bias, H, W, eps)``: the multi-scale feature tap of ``MM_FastVim``
  (models/fastvim.py:682-690) -- ``nn.LayerNorm`` over the channels of (B, H*W, C) hidden states (bf16 / fp32),
  returned as the fp32 (B, C, H, W) map in one launch.  Token ``l`` is cell ``(l // W, l % W)``.
* ``ln2d_fn(x, weight, bias, eps)``: the detection recipe's ``LN2d`` (detection/vitdet/simple_fpn.py:15-32), channel
  LayerNorm of a contiguous (N, C, H, W) map in ``x``'s dtype.

Both save the per-position ``mean`` / ``rstd`` for one backward launch.  Weight gradients follow the house convention:
a parameter flagged ``_fv_direct`` with a contiguous fp32 ``.grad`` view (``FlatTrainingState``) gets the per-workgroup
partial rows reduced straight into that view and autograd sees ``None``; otherwise the reduced gradient is returned.
GPU only: there is no fallback.
"""
import ctypes

import torch

from . import _lib as L
from .mixer_ops import reduce_partials


def _direct_view(param):
    g = param.grad
    if getattr(param, "_fv_direct", False) and g is not None and g.is_contiguous() and g.dtype == torch.float32 \
            and param.dtype == torch.float32:
        return g
    return None


def _weight_grads(pw, pb, nb, ctx):
    dw = db = None
    wdt, bdt = ctx.param_dtypes
    if ctx.w_direct is not None:
        reduce_partials(pw, nb, out=ctx.w_direct.view(-1), accumulate=True)
    elif ctx.needs_input_grad[1]:
        dw = reduce_partials(pw, nb).to(wdt)
    if ctx.needs_input_grad[2]:
        db = reduce_partials(pb, nb).to(bdt)
    return dw, db


def _affine(weight, bias, C, what):
    if weight is None or bias is None:
        raise RuntimeError(f"{what}: weight and bias are required (affine LayerNorm)")
    if weight.numel() != C or bias.numel() != C:
        raise RuntimeError(f"{what}: weight / bias have {weight.numel()} / {bias.numel()} elements, the input has C = {C}")
    return weight.detach().float().contiguous().view(-1), bias.detach().float().contiguous().view(-1)


def tap_ln_forward(hidden, weight, bias, H, W, eps=1e-5):
    """The tap's forward launch without autograd: returns (y fp32 (B, C, H, W), mean (B*H*W), rstd (B*H*W), and the
    contiguous input / fp32 weight the backward launch reads)."""
    L.require_gpu(hidden, weight, bias)
    if hidden.dim() != 3 or hidden.shape[1] != H * W:
        raise RuntimeError(f"tap_layer_norm_nchw: hidden {tuple(hidden.shape)} is not (B, H*W = {H * W}, C)")
    if hidden.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"tap_layer_norm_nchw: hidden must be fp32 or bf16, got {hidden.dtype}")
    B, Ltok, C = hidden.shape
    x = hidden.detach().contiguous()
    w32, b32 = _affine(weight, bias, C, "tap_layer_norm_nchw")
    dev = x.device
    y = torch.empty(B, C, H, W, device=dev, dtype=torch.float32)
    mean = torch.empty(B * Ltok, device=dev, dtype=torch.float32)
    rstd = torch.empty(B * Ltok, device=dev, dtype=torch.float32)
    rc = L.lib().fv_tap_ln_fwd(L.ptr(x), L.i32(L.dtype_code(x.dtype)), L.ptr(w32), L.ptr(b32), L.ptr(y), L.ptr(mean),
                               L.ptr(rstd), L.i32(B), L.i32(Ltok), L.i32(C), ctypes.c_float(eps), L.stream_of(x))
    L.check(rc, "tap_ln_fwd")
    return y, mean, rstd, x, w32


class TapLayerNormNCHWFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hidden, weight, bias, H, W, eps):
        y, mean, rstd, x, w32 = tap_ln_forward(hidden, weight, bias, H, W, eps)
        ctx.save_for_backward(x, w32, mean, rstd)
        ctx.w_direct = _direct_view(weight)
        ctx.param_dtypes = (weight.dtype, bias.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w32, mean, rstd = ctx.saved_tensors
        B, Ltok, C = x.shape
        dy = dy.float().contiguous()
        lib = L.lib()
        nb = lib.fv_tap_ln_blocks(L.i32(B), L.i32(Ltok))
        dx = torch.empty_like(x)
        pw = torch.empty(nb, C, device=x.device, dtype=torch.float32)
        pb = torch.empty(nb, C, device=x.device, dtype=torch.float32)
        rc = lib.fv_tap_ln_bwd(L.ptr(dy), L.ptr(x), L.i32(L.dtype_code(x.dtype)), L.ptr(w32), L.ptr(mean), L.ptr(rstd),
                               L.ptr(dx), L.ptr(pw), L.ptr(pb), L.i32(B), L.i32(Ltok), L.i32(C), L.stream_of(x))
        L.check(rc, "tap_ln_bwd")
        dw, db = _weight_grads(pw, pb, nb, ctx)
        return dx, dw, db, None, None, None


def ln2d_forward(x, weight, bias, eps=1e-6):
    """LN2d's forward launch without autograd: returns (y, mean (N*H*W), rstd (N*H*W), contiguous x, fp32 weight)."""
    L.require_gpu(x, weight, bias)
    if x.dim() != 4:
        raise RuntimeError(f"ln2d_fn: x {tuple(x.shape)} is not (N, C, H, W)")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"ln2d_fn: x must be fp32 or bf16, got {x.dtype}")
    N, C, H, W = x.shape
    xc = x.detach().contiguous()
    w32, b32 = _affine(weight, bias, C, "ln2d_fn")
    y = torch.empty_like(xc)
    mean = torch.empty(N * H * W, device=x.device, dtype=torch.float32)
    rstd = torch.empty(N * H * W, device=x.device, dtype=torch.float32)
    rc = L.lib().fv_ln2d_fwd(L.ptr(xc), L.i32(L.dtype_code(xc.dtype)), L.ptr(w32), L.ptr(b32), L.ptr(y), L.ptr(mean),
                             L.ptr(rstd), L.i32(N), L.i32(C), L.i32(H * W), ctypes.c_float(eps), L.stream_of(xc))
    L.check(rc, "ln2d_fwd")
    return y, mean, rstd, xc, w32


class LN2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        y, mean, rstd, xc, w32 = ln2d_forward(x, weight, bias, eps)
        ctx.save_for_backward(xc, w32, mean, rstd)
        ctx.w_direct = _direct_view(weight)
        ctx.param_dtypes = (weight.dtype, bias.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w32, mean, rstd = ctx.saved_tensors
        N, C, H, W = x.shape
        dy = dy.to(x.dtype).contiguous()
        lib = L.lib()
        nb = lib.fv_ln2d_blocks(L.i32(N), L.i32(C), L.i32(H * W))
        dx = torch.empty_like(x)
        pw = torch.empty(nb, C, device=x.device, dtype=torch.float32)
        pb = torch.empty(nb, C, device=x.device, dtype=torch.float32)
        rc = lib.fv_ln2d_bwd(L.ptr(dy), L.ptr(x), L.i32(L.dtype_code(x.dtype)), L.ptr(w32), L.ptr(mean), L.ptr(rstd),
                             L.ptr(dx), L.ptr(pw), L.ptr(pb), L.i32(N), L.i32(C), L.i32(H * W), L.stream_of(x))
        L.check(rc, "ln2d_bwd")
        dw, db = _weight_grads(pw, pb, nb, ctx)
        return dx, dw, db, None


def tap_layer_norm_nchw(hidden, weight, bias, H, W, eps=1e-5):
    """(B, H*W, C) hidden states -> fp32 (B, C, H, W) = LayerNorm over C, affine, in one launch."""
    return TapLayerNormNCHWFn.apply(hidden, weight, bias, int(H), int(W), float(eps))


def ln2d_fn(x, weight, bias, eps=1e-6):
    """Channel LayerNorm of a (N, C, H, W) map (``LN2d``), output in ``x``'s dtype."""
    return LN2dFn.apply(x, weight, bias, float(eps))
