"""Host wrappers of csrc/glue.hip: the small memory-bound ops around the backbone (patch unfold, patch projection with
the bias / position-embedding epilogue, token mean pool, the stochastic-depth table, loss-gradient scaling, bias
gradients).  Each is one HIP launch where the eager expression is a string of library kernels."""
import ctypes

import torch

from . import _lib as L
from .mixer_ops import reduce_partials


def patch_unfold(x, ph, pw, out_dtype):
    """(B, C, H, W) -> (B, gh*gw, C*ph*pw) in ``out_dtype``: the operand of the k == stride patch-embed conv as a GEMM
    (models/fastvim.py:95), unfolded and cast in one pass."""
    B, C, H, W = x.shape
    x = x.contiguous()
    out = torch.empty(B, (H // ph) * (W // pw), C * ph * pw, device=x.device, dtype=out_dtype)
    rc = L.lib().fv_patch_unfold(L.ptr(x), L.i32(L.dtype_code(x.dtype)), L.ptr(out), L.i32(L.dtype_code(out_dtype)),
                                 L.i32(B), L.i32(C), L.i32(H), L.i32(W), L.i32(ph), L.i32(pw), L.stream_of(x))
    L.check(rc, "patch_unfold")
    return out


def patch_unfold_ok(x, ph, pw):
    """Any even patch width from 8 up: multiples of 8 take the 16-byte form, the others (patch 14) the 2-element-pair form."""
    return (x.is_cuda and x.dim() == 4 and x.dtype in (torch.float32, torch.bfloat16) and pw % 2 == 0 and pw >= 8
            and x.shape[2] % ph == 0 and x.shape[3] % pw == 0 and x.shape[1] * ph * pw * 16 * 4 <= 64 * 1024)


def patch_unfold_chan_ok(x, ph, pw, n_sel):
    return (x.is_cuda and x.dim() == 4 and x.dtype in (torch.float32, torch.bfloat16) and pw % 8 == 0
            and x.shape[2] % ph == 0 and x.shape[3] % pw == 0 and n_sel * ph * pw * 4 <= 64 * 1024)


def patch_unfold_chan(x, ph, pw, out_dtype, sel, n_sel, colwise=False):
    """(B, Ctot, H, W) -> (B, P * n_sel, ph*pw) in ``out_dtype``, tokens in (row, col, channel) order (``colwise``: (col, row,
    channel)), channel k of the output = ``x[:, sel[k]]``: the per-channel patches of the shared projection, gathered,
    unfolded and cast in one pass.  ``sel``: int32 device tensor read when the kernel runs, or None (the first ``n_sel``
    channels)."""
    B, Ctot, H, W = x.shape
    x = x.contiguous()
    out = torch.empty(B, (H // ph) * (W // pw) * n_sel, ph * pw, device=x.device, dtype=out_dtype)
    rc = L.lib().fv_patch_unfold_chan(L.ptr(x), L.i32(L.dtype_code(x.dtype)), L.ptr(out), L.i32(L.dtype_code(out_dtype)),
                                      L.i32(B), L.i32(Ctot), L.i32(H), L.i32(W), L.i32(ph), L.i32(pw), L.ptr(sel), L.i32(n_sel),
                                      L.i32(bool(colwise)), L.stream_of(x))
    L.check(rc, "patch_unfold_chan")
    return out


def chan_embed_table(chan_table, bias, pos, sel, n_sel, positions):
    """fp32 (positions * n_sel, D): ``table[p * n_sel + k] = (chan_table[sel[k]] + bias) + pos[p]`` -- the per-token table
    the channel models' patch GEMM adds in its epilogue.  ``chan_table`` (Ctot, D), ``bias`` (D) or None, ``pos``
    (positions, D) or None, all fp32 and contiguous."""
    Ctot, D = chan_table.shape
    table = torch.empty(positions * n_sel, D, device=chan_table.device, dtype=torch.float32)
    rc = L.lib().fv_chan_embed_table(L.ptr(chan_table), L.ptr(bias), L.ptr(pos), L.ptr(table), L.ptr(sel), L.i32(n_sel),
                                     L.i32(Ctot), L.i32(positions), L.i32(D), L.stream_of(chan_table))
    L.check(rc, "chan_embed_table")
    return table


def chan_embed_scatter_(d_table, d_chan, sel):
    """In place: ``d_table[sel[k]] += d_chan[k]`` (fp32; ``sel`` None: k); the other rows are not touched."""
    n_sel, D = d_chan.shape
    rc = L.lib().fv_chan_embed_scatter(L.ptr(d_chan), L.ptr(d_table), L.ptr(sel), L.i32(n_sel), L.i32(d_table.shape[0]), L.i32(D),
                                       L.stream_of(d_chan))
    L.check(rc, "chan_embed_scatter")
    return d_table


def mix_batch(x, block, out=None):
    """Batch-mode Mixup / CutMix of (B, C, H, W) images, out of place: ``out[b] = mix(x[b], x[B-1-b])`` with the
    parameters the device ``block`` (fastvim_amd.mixup.Mixup.block) holds at the time the kernel runs.  One launch that
    reads the batch once and writes it once (timm: flip, mul_, mul_, add_)."""
    L.require_gpu(x, block)
    if x.dim() != 4 or x.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"mix_batch: expected (B, C, H, W) fp32 or bf16 images, got {tuple(x.shape)} {x.dtype}")
    B, C, H, W = x.shape
    x = x.contiguous()
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != x.dtype or not out.is_contiguous():
        raise RuntimeError("mix_batch: `out` must be a contiguous tensor of the input's shape and dtype")
    rc = L.lib().fv_mix_batch(L.ptr(x), L.ptr(out), L.i32(L.dtype_code(x.dtype)), L.i32(B), L.i32(C), L.i32(H), L.i32(W),
                              L.ptr(block), L.stream_of(x))
    L.check(rc, "mix_batch")
    return out


def patch_unfold_mix(x, ph, pw, out_dtype, block):
    """``patch_unfold`` of the mixed batch in one launch (the mixed images never exist in memory): bit for bit
    ``patch_unfold(mix_batch(x, block), ph, pw, out_dtype)``.  Applicable where ``patch_unfold_ok`` and the batch is even."""
    B, C, H, W = x.shape
    x = x.contiguous()
    out = torch.empty(B, (H // ph) * (W // pw), C * ph * pw, device=x.device, dtype=out_dtype)
    rc = L.lib().fv_patch_unfold_mix(L.ptr(x), L.i32(L.dtype_code(x.dtype)), L.ptr(out), L.i32(L.dtype_code(out_dtype)),
                                     L.i32(B), L.i32(C), L.i32(H), L.i32(W), L.i32(ph), L.i32(pw), L.ptr(block), L.stream_of(x))
    L.check(rc, "patch_unfold_mix")
    return out


# ---- 8-bit images: the unfolds above with the per-channel normalisation as a table lookup (csrc/unfold_u8.hip) ----------
# ``table``: the (C, 256) fp32 tensor of fastvim_amd.pixels.PixelNorm.table(device).  Each function is bit for bit the float
# function of the same name applied to ``table[c][x]`` as an fp32 image; the ``_u8_ok`` predicates are pure host functions
# of the tensor's shape, dtype, layout and address (a meta or CPU stand-in answers for the shape).

def _u8_images(x, align):
    # (is_cuda is the caller's check: the kernels run on the GPU only, the predicate also answers for a stand-in)
    return (x.dim() == 4 and x.dtype == torch.uint8 and x.is_contiguous()
            and (x.device.type == "meta" or x.data_ptr() % align == 0))


def patch_unfold_u8_ok(x, ph, pw):
    """Any even patch width from 8 up, 16 fp32 patches plus the table (1 KB per channel) within 64 KB of LDS, NCHW-contiguous
    images at an even address (16 pixels per load where width and address allow, down to 2)."""
    return (_u8_images(x, 2) and pw % 2 == 0 and pw >= 8 and x.shape[2] % ph == 0 and x.shape[3] % pw == 0
            and x.shape[1] * (ph * pw * 16 * 4 + 1024) <= 64 * 1024)


def patch_unfold_chan_u8_ok(x, ph, pw, n_sel):
    return (_u8_images(x, 4) and pw % 8 == 0 and x.shape[2] % ph == 0 and x.shape[3] % pw == 0
            and 0 < n_sel <= x.shape[1] and n_sel * (ph * pw * 4 + 1024) <= 64 * 1024)


def _u8_table(x, table, rows):
    L.require_gpu(x, table)
    if table.dtype != torch.float32 or tuple(table.shape) != (rows, 256) or not table.is_contiguous() or table.device != x.device:
        raise RuntimeError(f"pixel table: expected a contiguous fp32 ({rows}, 256) tensor on {x.device}, got "
                           f"{tuple(table.shape)} {table.dtype} on {table.device}")


def patch_unfold_u8(x, table, ph, pw, out_dtype):
    """uint8 (B, C, H, W) -> (B, gh*gw, C*ph*pw) in ``out_dtype``: ``patch_unfold(table[c][x], ph, pw, out_dtype)`` in one
    launch that reads a quarter of the image bytes."""
    B, C, H, W = x.shape
    _u8_table(x, table, C)
    out = torch.empty(B, (H // ph) * (W // pw), C * ph * pw, device=x.device, dtype=out_dtype)
    rc = L.lib().fv_patch_unfold_u8(L.ptr(x), L.ptr(table), L.ptr(out), L.i32(L.dtype_code(out_dtype)), L.i32(B), L.i32(C),
                                    L.i32(H), L.i32(W), L.i32(ph), L.i32(pw), L.stream_of(x))
    L.check(rc, "patch_unfold_u8")
    return out


def patch_unfold_mix_u8(x, table, ph, pw, out_dtype, block):
    """``patch_unfold_mix(table[c][x], ph, pw, out_dtype, block)``: the pixels are looked up, then mixed in fp32 with the
    float kernel's expressions.  Applicable where ``patch_unfold_u8_ok`` and the batch is even."""
    B, C, H, W = x.shape
    _u8_table(x, table, C)
    out = torch.empty(B, (H // ph) * (W // pw), C * ph * pw, device=x.device, dtype=out_dtype)
    rc = L.lib().fv_patch_unfold_mix_u8(L.ptr(x), L.ptr(table), L.ptr(out), L.i32(L.dtype_code(out_dtype)), L.i32(B), L.i32(C),
                                        L.i32(H), L.i32(W), L.i32(ph), L.i32(pw), L.ptr(block), L.stream_of(x))
    L.check(rc, "patch_unfold_mix_u8")
    return out


def patch_unfold_chan_u8(x, table, ph, pw, out_dtype, sel, n_sel, colwise=False):
    """``patch_unfold_chan(table[c][x], ...)``: output channel k is looked up in row ``sel[k]`` of the table -- the SOURCE
    channel's statistics (``sel`` None: row k)."""
    B, Ctot, H, W = x.shape
    _u8_table(x, table, Ctot)
    out = torch.empty(B, (H // ph) * (W // pw) * n_sel, ph * pw, device=x.device, dtype=out_dtype)
    rc = L.lib().fv_patch_unfold_chan_u8(L.ptr(x), L.ptr(table), L.ptr(out), L.i32(L.dtype_code(out_dtype)), L.i32(B), L.i32(Ctot),
                                         L.i32(H), L.i32(W), L.i32(ph), L.i32(pw), L.ptr(sel), L.i32(n_sel),
                                         L.i32(bool(colwise)), L.stream_of(x))
    L.check(rc, "patch_unfold_chan_u8")
    return out


# ---- random erasing (csrc/erase.hip, the ERASE forms of csrc/unfold_u8.hip) ----------------------------------------------
# ``block``: the int32 erase block of fastvim_amd.erasing.RandomErasing.block(device) -- boxes, mode and noise key, read when
# the kernel runs.

def _erase_block(x, block):
    L.require_gpu(x, block)
    if (block.dtype != torch.int32 or block.dim() != 1 or not block.is_contiguous() or block.device != x.device
            or block.numel() < 4 + 4 * x.shape[0] or block.data_ptr() % 16 != 0):
        raise RuntimeError(f"erase block: expected a contiguous, 16-byte aligned int32 tensor of at least 4 + 4 * {x.shape[0]} "
                           f"entries on {x.device}, got {tuple(block.shape)} {block.dtype} on {block.device}")


def random_erase(x, block, out=None):
    """Random erasing of (B, C, H, W) fp32 / bf16 images with the boxes and the noise key the device ``block`` holds at the
    time the kernel runs: ``out`` = ``x`` outside the boxes, 0 or standard-normal noise inside.  Out of place by default;
    ``out=x`` erases in place (only the boxes are touched)."""
    if x.dim() != 4 or x.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"random_erase: expected (B, C, H, W) fp32 or bf16 images, got {tuple(x.shape)} {x.dtype}")
    _erase_block(x, block)
    B, C, H, W = x.shape
    if out is x:
        if not x.is_contiguous():
            raise RuntimeError("random_erase: in place needs a contiguous batch")
    else:
        x = x.contiguous()
        if out is None:
            out = torch.empty_like(x)
        elif out.shape != x.shape or out.dtype != x.dtype or not out.is_contiguous() or out.device != x.device:
            raise RuntimeError("random_erase: `out` must be a contiguous tensor of the input's shape, dtype and device")
    rc = L.lib().fv_random_erase(L.ptr(x), L.ptr(out), L.i32(L.dtype_code(x.dtype)), L.i32(B), L.i32(C), L.i32(H), L.i32(W),
                                 L.ptr(block), L.stream_of(x))
    L.check(rc, "random_erase")
    return out


def patch_unfold_u8_re(x, table, ph, pw, out_dtype, erase):
    """``patch_unfold(random_erase(table[c][x], erase), ph, pw, out_dtype)`` in the one launch of ``patch_unfold_u8``: the
    pixels inside a sample's box are replaced between the lookup and the placement.  Applicable where
    ``patch_unfold_u8_ok``."""
    B, C, H, W = x.shape
    _u8_table(x, table, C)
    _erase_block(x, erase)
    out = torch.empty(B, (H // ph) * (W // pw), C * ph * pw, device=x.device, dtype=out_dtype)
    rc = L.lib().fv_patch_unfold_u8_re(L.ptr(x), L.ptr(table), L.ptr(out), L.i32(L.dtype_code(out_dtype)), L.i32(B), L.i32(C),
                                       L.i32(H), L.i32(W), L.i32(ph), L.i32(pw), L.ptr(erase), L.stream_of(x))
    L.check(rc, "patch_unfold_u8_re")
    return out


def patch_unfold_mix_u8_re(x, table, ph, pw, out_dtype, block, erase):
    """``patch_unfold_mix(random_erase(table[c][x], erase), ph, pw, out_dtype, block)``: each image of a pair is erased
    with its own box, then the two are mixed.  Applicable where ``patch_unfold_u8_ok`` and the batch is even."""
    B, C, H, W = x.shape
    _u8_table(x, table, C)
    _erase_block(x, erase)
    out = torch.empty(B, (H // ph) * (W // pw), C * ph * pw, device=x.device, dtype=out_dtype)
    rc = L.lib().fv_patch_unfold_mix_u8_re(L.ptr(x), L.ptr(table), L.ptr(out), L.i32(L.dtype_code(out_dtype)), L.i32(B), L.i32(C),
                                           L.i32(H), L.i32(W), L.i32(ph), L.i32(pw), L.ptr(block), L.ptr(erase), L.stream_of(x))
    L.check(rc, "patch_unfold_mix_u8_re")
    return out


def gemm_rowbias(a, w, table):
    """fp32 (M, N) = bf16_round(a (M, K) @ w (N, K)^T) + table[m mod period]: bf16 operands, table (period, N) fp32."""
    M, K = a.shape
    N = w.shape[0]
    period = table.shape[0]
    c = torch.empty(M, N, device=a.device, dtype=torch.float32)
    rc = L.lib().fv_gemm_bf16_rowbias(L.ptr(a), L.ptr(w), L.ptr(c), L.ptr(table), L.i32(period), L.i32(M), L.i32(N), L.i32(K),
                                      ctypes.c_long(a.stride(0)), ctypes.c_long(w.stride(0)), ctypes.c_long(N), L.stream_of(a))
    L.check(rc, "gemm_bf16_rowbias")
    return c


class MeanPoolFn(torch.autograd.Function):
    """x (B, L, D) -> (B, D): ``x.mean(dim=1)`` (models/fastvim.py:529-531) and its adjoint, one launch each."""

    @staticmethod
    def forward(ctx, x):
        L.require_gpu(x)
        B, Ltok, D = x.shape
        xc = x.contiguous()
        out = torch.empty(B, D, device=x.device, dtype=x.dtype)
        rc = L.lib().fv_mean_pool_fwd(L.ptr(xc), L.ptr(out), L.i32(B), L.i32(Ltok), L.i32(D), L.i32(L.dtype_code(x.dtype)),
                                      L.stream_of(xc))
        L.check(rc, "mean_pool_fwd")
        ctx.shape = (B, Ltok, D)
        return out

    @staticmethod
    def backward(ctx, g):
        B, Ltok, D = ctx.shape
        g = g.contiguous()
        dx = torch.empty(B, Ltok, D, device=g.device, dtype=g.dtype)
        rc = L.lib().fv_mean_pool_bwd(L.ptr(g), L.ptr(dx), L.i32(B), L.i32(Ltok), L.i32(D), L.i32(L.dtype_code(g.dtype)),
                                      L.stream_of(g))
        L.check(rc, "mean_pool_bwd")
        return dx


def mean_pool_ok(x):
    return x.is_cuda and x.dim() == 3 and x.dtype in (torch.float32, torch.bfloat16) and x.shape[2] % 4 == 0


def droppath_table_(table, keep, inv_keep):
    """In place: U[0,1) draws (mods, batch) -> floor(keep + U) * inv_keep, one row of per-sample scales per module."""
    mods, batch = table.shape
    rc = L.lib().fv_droppath_table(L.ptr(table), L.ptr(keep), L.ptr(inv_keep), L.i32(mods), L.i32(batch), L.stream_of(table))
    L.check(rc, "droppath_table")
    return table


def scale_cast(x, scale, out_dtype):
    """x (fp32) * scale (0-dim / 1-element fp32 device tensor), cast to ``out_dtype``."""
    x = x.contiguous()
    y = torch.empty(x.shape, device=x.device, dtype=out_dtype)
    rc = L.lib().fv_scale_cast(L.ptr(x), L.ptr(scale), L.ptr(y), L.i32(L.dtype_code(out_dtype)), ctypes.c_size_t(x.numel()),
                               L.stream_of(x))
    L.check(rc, "scale_cast")
    return y


def column_sum(x, out=None, accumulate=False):
    """Sum over the rows of a (rows, cols) fp32 / bf16 matrix -> (cols,) fp32 (fixed order); ``out`` + ``accumulate`` add
    into a gradient buffer."""
    rows, cols = x.shape
    x = x.contiguous()
    if out is None:
        out = torch.empty(cols, device=x.device, dtype=torch.float32)
        accumulate = False
    rc = L.lib().fv_column_sum(L.ptr(x), L.i32(L.dtype_code(x.dtype)), L.ptr(out), L.i32(rows), L.i32(cols), L.i32(accumulate),
                               L.stream_of(x))
    L.check(rc, "column_sum")
    return out
