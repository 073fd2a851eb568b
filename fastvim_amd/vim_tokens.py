"""The class token of the supervised Vim baseline on the HIP path (``fastvim_amd.vim.VisionMamba.fused_cls``).

``cls_tokens`` (csrc/vim_tokens.hip) puts the class token among the patch tokens and adds the position table: one launch
where ``forward_features`` runs ``expand / to / cat / +`` -- and one launch backward where autograd runs slice copies and two
sums over the batch.  ``add_norm_row`` (csrc/norm.hip, the row kernels) is the model's tail -- DropPath scale, residual add
and RMSNorm / LayerNorm -- of the ONE row per sample that the head reads, where ``forward_features`` normalises all
``B (M + 1)`` rows and selects; its backward writes the whole ``d hidden`` / ``d residual`` (zero outside the row) itself.

Values equal the torch chains bit for bit.  What differs is the order of three sums -- ``pos_embed.grad`` and
``cls_token.grad`` (here in fp64 in the order of the samples, rounded once) and the norm's ``weight.grad`` / ``bias.grad``
(fixed-order fp32 sums over the B rows instead of all rows, the others contributing exact zeros).

``*_ok`` are pure Python: no GPU and no library needed to ask.  The ops raise where their predicate says no; ``assemble``
and the model choose the torch chain there.  Nothing here synchronises with the host; outputs are allocated by torch on the
current stream: safe under graph capture.
"""
import ctypes

import torch

from . import _lib as L
from .mixer_ops import reduce_partials

_DTYPES = (torch.float32, torch.bfloat16)
MAX_NORM_DIM = 2048              # csrc/norm.hip: MAXK_LIMIT * 256


def _table_ok(t, numel, ref):
    return (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.numel() == numel and t.is_contiguous()
            and t.device == ref.device)


def cls_tokens_ok(y, cls_token, pos_embed, position):
    """Whether ``cls_tokens`` takes these arguments: ``y`` (B, M, D) fp32 or bf16, contiguous, on the GPU, D % 4 == 0;
    ``cls_token`` D fp32 values and ``pos_embed`` (M + 1) D fp32 values, contiguous, on y's device; 0 <= position <= M."""
    if not isinstance(y, torch.Tensor) or y.dim() != 3 or not y.is_cuda or y.dtype not in _DTYPES or not y.is_contiguous():
        return False
    B, M, D = y.shape
    if B <= 0 or M <= 0 or D <= 0 or D % 4 != 0 or B * (M + 1) >= 2 ** 31:
        return False
    return _table_ok(cls_token, D, y) and _table_ok(pos_embed, (M + 1) * D, y) and 0 <= int(position) <= M


def cls_tokens_chain(y, cls_token, pos_embed, position):
    """The torch chain of ``forward_features`` that ``cls_tokens`` stands for."""
    cls = cls_token.expand(y.shape[0], -1, -1).to(y.dtype)
    return torch.cat((y[:, :position, :], cls, y[:, position:, :]), dim=1) + pos_embed


class _ClsTokensFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, cls_token, pos_embed, position):
        B, M, D = y.shape
        out = torch.empty(B, M + 1, D, device=y.device, dtype=torch.float32)
        rc = L.lib().fv_vim_cls_tokens_fwd(L.ptr(y), L.i32(L.dtype_code(y.dtype)), L.ptr(cls_token), L.ptr(pos_embed), L.ptr(out),
                                           L.i32(B), L.i32(M), L.i32(D), L.i32(position), L.stream_of(y))
        L.check(rc, "vim_cls_tokens_fwd")
        ctx.geo = (B, M, D, position, y.dtype, tuple(cls_token.shape), tuple(pos_embed.shape))
        return out

    @staticmethod
    def backward(ctx, dout):
        B, M, D, position, y_dtype, ct_shape, pe_shape = ctx.geo
        dout = dout.float().contiguous()
        dy = torch.empty(B, M, D, device=dout.device, dtype=y_dtype)
        dpos = torch.empty(M + 1, D, device=dout.device, dtype=torch.float32)
        dcls = torch.empty(D, device=dout.device, dtype=torch.float32)
        rc = L.lib().fv_vim_cls_tokens_bwd(L.ptr(dout), L.ptr(dy), L.i32(L.dtype_code(y_dtype)), L.ptr(dpos), L.ptr(dcls), L.i32(B),
                                           L.i32(M), L.i32(D), L.i32(position), L.stream_of(dout))
        L.check(rc, "vim_cls_tokens_bwd")
        return dy, dcls.view(ct_shape), dpos.view(pe_shape), None


def cls_tokens(y, cls_token, pos_embed, position):
    """``y`` (B, M, D) fp32 or bf16, the patch projection with the conv bias added; ``cls_token`` (1, 1, D) fp32;
    ``pos_embed`` (1, M + 1, D) fp32; ``position`` the class token's row -> (B, M + 1, D) fp32: row j is
    ``(cls_token.to(y.dtype) if j == position else y[:, j - (j > position)]) + pos_embed[:, j]`` -- the values of
    ``cls_tokens_chain``, bit for bit (one fp32 add).  Backward: ``dy`` bit-identical to autograd's; ``d pos_embed`` and
    ``d cls_token`` the sums over the batch in fp64 in the order of the samples, rounded once to fp32."""
    if not cls_tokens_ok(y, cls_token, pos_embed, position):
        raise RuntimeError(f"cls_tokens: unsupported arguments (y {tuple(y.shape)} {y.dtype} on {y.device}, cls_token "
                           f"{tuple(cls_token.shape)} {cls_token.dtype}, pos_embed {tuple(pos_embed.shape)} {pos_embed.dtype}, "
                           f"position {position}); see cls_tokens_ok")
    return _ClsTokensFn.apply(y, cls_token, pos_embed, int(position))


def assemble(y, cls_token, pos_embed, position):
    """``cls_tokens`` where its predicate holds, the torch chain elsewhere: the same values either way."""
    if cls_tokens_ok(y, cls_token, pos_embed, position):
        return _ClsTokensFn.apply(y, cls_token, pos_embed, int(position))
    return cls_tokens_chain(y, cls_token, pos_embed, position)


# ------------------------------------------------------------------------------------------------- the tail: one row
def add_norm_row_ok(hidden, residual, weight, bias, position, row_scale=None, residual_in_fp32=True):
    """Whether ``add_norm_row`` takes these arguments: ``hidden`` (B, T, D) fp32 or bf16 and ``residual`` (B, T, D) fp32,
    both contiguous on the GPU, D % 4 == 0 and D <= 2048, ``residual_in_fp32``; ``weight`` (and ``bias``) D values on that
    device; 0 <= position < T; ``row_scale`` None or B values."""
    if not isinstance(hidden, torch.Tensor) or hidden.dim() != 3 or not hidden.is_cuda or hidden.dtype not in _DTYPES:
        return False
    if not hidden.is_contiguous() or not residual_in_fp32:
        return False
    B, T, D = hidden.shape
    if B <= 0 or T <= 0 or D <= 0 or D % 4 != 0 or D > MAX_NORM_DIM or B * T >= 2 ** 31 or not 0 <= int(position) < T:
        return False
    if (not isinstance(residual, torch.Tensor) or residual.shape != hidden.shape or residual.dtype != torch.float32
            or not residual.is_contiguous() or residual.device != hidden.device):
        return False
    for t in (weight, bias):
        if t is not None and (t.numel() != D or t.device != hidden.device or not t.is_floating_point()):
            return False
    if weight is None:
        return False
    return row_scale is None or (row_scale.numel() == B and row_scale.device == hidden.device)


def add_norm_row_backward(dy, r, weight, mean, rstd, row_scale, rows, position, is_rms_norm, hidden_dtype, has_bias,
                          dhidden=None, dresidual=None):
    """The one backward launch and the two partial reductions: ``dy`` (B, D), ``r`` (B, D) the normalised input,
    ``mean`` / ``rstd`` (B) as the forward left them -> (d hidden (B, rows, D) ``hidden_dtype``, d residual (B, rows, D)
    fp32, d weight, d bias).  ``dhidden`` / ``dresidual``: buffers to write into instead of fresh ones (every element of
    them is written)."""
    B, D = r.shape
    dev = r.device
    dy = dy.contiguous()
    if dhidden is None:
        dhidden = torch.empty(B, rows, D, device=dev, dtype=hidden_dtype)
    if dresidual is None:
        dresidual = torch.empty(B, rows, D, device=dev, dtype=torch.float32)
    lib = L.lib()
    nb = lib.fv_add_norm_blocks(L.i32(B))
    pw = torch.empty(nb, D, device=dev, dtype=torch.float32)
    pb = torch.empty(nb, D, device=dev, dtype=torch.float32) if has_bias else None
    rc = lib.fv_add_norm_row_bwd(L.ptr(dy), L.i32(L.dtype_code(dy.dtype)), L.ptr(r), L.i32(L.dtype_code(r.dtype)), L.ptr(weight),
                                 L.ptr(mean), L.ptr(rstd), L.ptr(row_scale), L.ptr(dhidden), L.i32(L.dtype_code(dhidden.dtype)),
                                 L.ptr(dresidual), L.i32(L.dtype_code(dresidual.dtype)), L.ptr(pw), L.ptr(pb), L.i32(B),
                                 L.i32(rows), L.i32(position), L.i32(D), L.i32(is_rms_norm), L.stream_of(r))
    L.check(rc, "add_norm_row_bwd")
    return dhidden, dresidual, reduce_partials(pw, nb), (reduce_partials(pb, nb) if has_bias else None)


class _AddNormRowFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hidden, residual, weight, bias, eps, position, row_scale, is_rms_norm):
        B, T, D = hidden.shape
        dev = hidden.device
        weight = weight.float().contiguous()
        bias = bias.float().contiguous() if bias is not None else None
        row_scale = row_scale.float().contiguous() if row_scale is not None else None
        y = torch.empty(B, D, device=dev, dtype=hidden.dtype)
        r = torch.empty(B, D, device=dev, dtype=torch.float32)          # residual_out of the row: the normalised input
        mean = None if is_rms_norm else torch.empty(B, device=dev, dtype=torch.float32)
        rstd = torch.empty(B, device=dev, dtype=torch.float32)
        rc = L.lib().fv_add_norm_row_fwd(L.ptr(hidden), L.i32(L.dtype_code(hidden.dtype)), L.ptr(residual),
                                         L.i32(L.dtype_code(residual.dtype)), L.ptr(weight), L.ptr(bias), L.ptr(row_scale), L.ptr(y),
                                         L.i32(L.dtype_code(y.dtype)), L.ptr(r), L.i32(L.dtype_code(r.dtype)), L.ptr(mean),
                                         L.ptr(rstd), L.i32(B), L.i32(T), L.i32(position), L.i32(D), ctypes.c_float(eps),
                                         L.i32(is_rms_norm), L.stream_of(hidden))
        L.check(rc, "add_norm_row_fwd")
        ctx.save_for_backward(r, weight, bias, mean, rstd, row_scale)
        ctx.geo = (T, position, bool(is_rms_norm), hidden.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        r, weight, bias, mean, rstd, row_scale = ctx.saved_tensors
        T, position, is_rms_norm, hidden_dtype = ctx.geo
        dh, dr, dw, db = add_norm_row_backward(dy, r, weight, mean, rstd, row_scale, T, position, is_rms_norm, hidden_dtype,
                                               bias is not None)
        return dh, dr, dw, db, None, None, None, None


def add_norm_row(hidden, residual, weight, bias, eps, position, row_scale=None, is_rms_norm=False, residual_in_fp32=True):
    """``layer_norm_fn(hidden, weight, bias, residual=residual, eps=eps, prenorm=False, residual_in_fp32=True,
    is_rms_norm=is_rms_norm, row_scale=row_scale)[:, position]`` -- (B, D) in ``hidden``'s dtype, bit for bit -- computed for
    that row alone.  Backward: ``d hidden`` / ``d residual`` (B, T, D) from ONE launch, row ``position`` bit-identical to
    the whole-sequence backward, exact zeros elsewhere; ``d weight`` / ``d bias`` fixed-order sums over the B rows."""
    if not add_norm_row_ok(hidden, residual, weight, bias, position, row_scale, residual_in_fp32):
        raise RuntimeError(f"add_norm_row: unsupported arguments (hidden {tuple(hidden.shape)} {hidden.dtype} on {hidden.device}, "
                           f"residual {None if residual is None else (tuple(residual.shape), residual.dtype)}, position "
                           f"{position}, residual_in_fp32 {residual_in_fp32}); see add_norm_row_ok")
    return _AddNormRowFn.apply(hidden, residual, weight, bias, float(eps), int(position), row_scale, bool(is_rms_norm))
