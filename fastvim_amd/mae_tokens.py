"""Token bookkeeping of the MAE masked encoder on the HIP path (csrc/mae_tokens.hip; ``MaskedAutoencoderViM.fused_tokens``).

Everything ``random_masking``, the odd ``Block_masked`` layers and the masked mixers derive from the (N, L) masking noise --
which tokens are kept, the unshuffle index, the mask, the kept tokens' order in the transposed grid and its inverse, the
mixers' (2, B, K) row indices of both layer parities -- comes from ONE launch per step (``mask_plan`` -> ``TokenPlan``).  The
row copies that use it (``gather_tokens``: the masking gather, the odd layers' permute and un-permute) and the decoder's input
assembly (``decoder_tokens``) are ``autograd.Function``s over plain gather kernels: the indices are unique, so the adjoint of
a gather is the gather by the inverse index -- one pass, no zero fill, no atomics, and bit-identical to the
``torch.gather`` composition and its autograd.  The one value that is not bit-identical is the gradient of ``mask_token``: a
sum over the removed rows, here in fp64 in a fixed order (deterministic), in eager in whatever order the reduction takes.

The Vim MAE baseline (fastvim_amd/fastvim_mae.py) carries a class token -- in the middle of the kept tokens in the encoder,
behind the grid in the decoder: ``encoder_tokens_cls`` and ``decoder_tokens_cls`` (csrc/mae_tokens_cls.hip) are its two
assemblies, one launch each way, on the same plan.

Nothing here synchronises with the host; outputs are allocated by torch on the current stream: safe under graph capture.
"""
import struct
from typing import NamedTuple

import torch

from . import _lib as L
from ._devblock import BlockWriter

_M64 = (1 << 64) - 1
MAX_TOKENS = 1024               # FV_MAE_PLAN_MAX_TOKENS: 32 x 32, FastVim-H at 448 px
MIN_KEEP = 3                     # the masked mixer's conv halo
DECODER_ROWS_PER_BLOCK = 32      # FV_MAE_DECODER_ROWS_PER_BLOCK
_DTYPES = (torch.float32, torch.bfloat16)


class TokenPlan(NamedTuple):
    """What one ``fv_mae_mask_plan`` launch writes; B samples, L = H W tokens, K kept.  The int64 tensors are what the eager
    model computes (and returns); the int32 ones feed the kernels."""
    ids_keep: torch.Tensor          # (B, K) int64, ascending positions of the kept tokens
    ids_restore: torch.Tensor       # (B, L) int64: a kept token's place among the kept ones, a removed token's rank
    mask: torch.Tensor              # (B, L) fp32, 1 = removed
    keep_index: torch.Tensor        # (B, K) int32 = ids_keep
    restore_index: torch.Tensor     # (B, L) int32 = ids_restore where < K, else -1
    row_index_even: torch.Tensor    # (2, B, K) int32: the even mixers' [r, (H - 1) - flip(r)], r = ids_keep // W
    ids_keep_odd: torch.Tensor      # (B, K) int64: the kept tokens' places in the transposed grid, ascending
    order: torch.Tensor             # (B, K) int64: kept tokens in the transposed grid's scan order
    inverse: torch.Tensor           # (B, K) int64: argsort(order)
    order_index: torch.Tensor       # (B, K) int32 = order
    inverse_index: torch.Tensor     # (B, K) int32 = inverse
    row_index_odd: torch.Tensor     # (2, B, K) int32: the odd mixers' [r, (W - 1) - flip(r)], r = ids_keep_odd // H
    token_size: tuple               # (H, W)


def mask_plan_ok(noise, token_size, len_keep):
    """Whether ``mask_plan`` takes these arguments: (N, L) fp32 contiguous noise on the GPU, L = H W <= 1024,
    3 <= len_keep <= L.  Pure Python: no GPU and no library needed to ask."""
    H, W = int(token_size[0]), int(token_size[1])
    if not isinstance(noise, torch.Tensor) or noise.dim() != 2 or not noise.is_cuda:
        return False
    if noise.dtype != torch.float32 or not noise.is_contiguous() or noise.data_ptr() % 4 != 0:
        return False
    N, Ln = noise.shape
    if N <= 0 or H <= 0 or W <= 0 or Ln != H * W or Ln > MAX_TOKENS:
        return False
    return MIN_KEEP <= int(len_keep) <= Ln


def mask_plan(noise, token_size, len_keep):
    """The masking plan of ``noise`` (N, L): one launch.  The K = ``len_keep`` tokens of lowest noise are kept, ties broken
    by position (``torch.argsort(stable=True)``).  Finite noise is the contract; NaN noise gives an unspecified plan whose
    indices are still all in range.  Raises where ``mask_plan_ok`` says no: the caller chooses the fallback."""
    if not mask_plan_ok(noise, token_size, len_keep):
        raise RuntimeError(f"mask_plan: unsupported arguments (noise {tuple(noise.shape)} {noise.dtype} on {noise.device}, "
                           f"token_size {tuple(token_size)}, len_keep {len_keep}); see mask_plan_ok")
    H, W, K = int(token_size[0]), int(token_size[1]), int(len_keep)
    noise = noise.detach()
    N, Ln = noise.shape
    plan = _empty_plan(N, H, W, K, noise.device)
    rc = L.lib().fv_mae_mask_plan(L.ptr(noise), L.ptr(plan.ids_keep), L.ptr(plan.ids_restore), L.ptr(plan.mask),
                                  L.ptr(plan.keep_index), L.ptr(plan.restore_index), L.ptr(plan.row_index_even),
                                  L.ptr(plan.ids_keep_odd), L.ptr(plan.order), L.ptr(plan.inverse), L.ptr(plan.order_index),
                                  L.ptr(plan.inverse_index), L.ptr(plan.row_index_odd), L.i32(N), L.i32(H), L.i32(W), L.i32(K),
                                  L.stream_of(noise))
    L.check(rc, "mae_mask_plan")
    return plan


def plan_shape_ok(batch, token_size, len_keep):
    """The part of the plan's predicate that is about sizes: ``batch`` >= 1, an (H, W) grid of at most 1024 tokens,
    3 <= len_keep <= H W.  What ``mask_plan_keyed`` asks (it has no noise tensor to check).  Pure Python."""
    H, W = int(token_size[0]), int(token_size[1])
    if int(batch) <= 0 or H <= 0 or W <= 0 or H * W > MAX_TOKENS:
        return False
    return MIN_KEEP <= int(len_keep) <= H * W


def _empty_plan(N, H, W, K, dev):
    Ln = H * W
    i64 = lambda *s: torch.empty(*s, device=dev, dtype=torch.int64)
    i32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.int32)
    return TokenPlan(ids_keep=i64(N, K), ids_restore=i64(N, Ln), mask=torch.empty(N, Ln, device=dev, dtype=torch.float32),
                     keep_index=i32(N, K), restore_index=i32(N, Ln), row_index_even=i32(2, N, K), ids_keep_odd=i64(N, K),
                     order=i64(N, K), inverse=i64(N, K), order_index=i32(N, K), inverse_index=i32(N, K),
                     row_index_odd=i32(2, N, K), token_size=(H, W))


class MaskSampler:
    """The MAE masking noise as a function of ``(seed, counter, sample, token)`` instead of a draw from torch's generator: the
    same masks on any device, after a resume, and from the CPU (tests/mask_noise_ref.py restates it in numpy).

    The noise of sample b, token l is ``float(w >> 8) * 2**-24`` with ``w`` word ``l & 3`` of Philox4x32-10 under key
    ``(seed & 0xffffffff, seed >> 32)`` and counter ``(l >> 2, b, counter & 0xffffffff, counter >> 32)`` (csrc/mask_noise.h).
    The four words ``(k0, k1, step_lo, step_hi)`` live in a KEY BLOCK in device memory that the kernels read when they RUN:
    ``sample()`` advances the 64-bit counter (from 0: the first masks are those of counter 1) and rewrites the block from
    pinned memory on the current stream, so a replayed graph masks with the counter of the last ``sample()`` -- the technique
    of ``Mixup.sample()`` and ``RandomErasing.sample()``.  Data-parallel ranks pass DIFFERENT seeds (``seed=rank``).  torch's
    generators are never touched."""

    def __init__(self, seed=0):
        self.seed, self.counter = int(seed) & _M64, 0
        self._block = None
        self._writer = None

    # ------------------------------------------------------------------ host side
    def words(self):
        """``(k0, k1, step_lo, step_hi)``: the key block for the current ``(seed, counter)``, four 32-bit words."""
        return (self.seed & 0xffffffff, self.seed >> 32, self.counter & 0xffffffff, self.counter >> 32)

    def sample(self):
        """Advance the counter -- new masks for the next step -- and write the block.  Returns ``last()``."""
        self.counter = (self.counter + 1) & _M64
        self._write()
        return self.last()

    def last(self):
        """``(seed, counter)`` of the masks the next launch takes."""
        return self.seed, self.counter

    def set_counter(self, n):
        self.counter = int(n) & _M64
        self._write()

    def state_dict(self):
        return {"seed": self.seed, "counter": self.counter}

    def load_state_dict(self, state):
        self.seed, self.counter = int(state["seed"]) & _M64, int(state["counter"]) & _M64
        self._write()

    # ------------------------------------------------------------------ device side
    def block(self, device=None):
        """The device key block (int32[4]), created on first use and rewritten by every ``sample()`` from then on."""
        if self._block is None:
            device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            if device.type != "cuda":
                raise RuntimeError("fastvim_amd ops run on the GPU only (HIP kernels); the key block needs a GPU device")
            self._block = torch.zeros(4, device=device, dtype=torch.int32)
            self._writer = BlockWriter(4)
            self._write()
        elif device is not None and torch.device(device).type == "cuda" and torch.device(device).index not in (None, self._block.device.index):
            raise RuntimeError(f"MaskSampler: the key block lives on {self._block.device}, the tensors on {device}")
        return self._block

    def _write(self):
        if self._block is None:
            return
        # an asynchronous copy from pinned memory on the current stream, no host wait (fastvim_amd/_devblock.py)
        self._writer.write(self._block, struct.pack("<4I", *self.words()))

    def noise(self, B, Ln, device=None):
        """The (B, L) fp32 noise of the current ``(seed, counter)``: one ``fv_mae_noise`` launch."""
        blk = self.block(device)
        out = torch.empty(int(B), int(Ln), device=blk.device, dtype=torch.float32)
        rc = L.lib().fv_mae_noise(L.ptr(blk), L.ptr(out), L.i32(B), L.i32(Ln), L.stream_of(out))
        L.check(rc, "mae_noise")
        return out


def mask_plan_keyed(sampler, batch, token_size, len_keep, device=None):
    """``mask_plan(sampler.noise(batch, H W), token_size, len_keep)`` from ONE launch in which the noise never reaches
    memory (``fv_mae_mask_plan_keyed``): every field bit for bit the same.  Raises where ``plan_shape_ok`` says no."""
    if not plan_shape_ok(batch, token_size, len_keep):
        raise RuntimeError(f"mask_plan_keyed: unsupported arguments (batch {batch}, token_size {tuple(token_size)}, "
                           f"len_keep {len_keep}); see plan_shape_ok")
    N, H, W, K = int(batch), int(token_size[0]), int(token_size[1]), int(len_keep)
    blk = sampler.block(device)
    plan = _empty_plan(N, H, W, K, blk.device)
    rc = L.lib().fv_mae_mask_plan_keyed(L.ptr(blk), L.ptr(plan.ids_keep), L.ptr(plan.ids_restore), L.ptr(plan.mask),
                                        L.ptr(plan.keep_index), L.ptr(plan.restore_index), L.ptr(plan.row_index_even),
                                        L.ptr(plan.ids_keep_odd), L.ptr(plan.order), L.ptr(plan.inverse),
                                        L.ptr(plan.order_index), L.ptr(plan.inverse_index), L.ptr(plan.row_index_odd),
                                        L.i32(N), L.i32(H), L.i32(W), L.i32(K), L.stream_of(plan.mask))
    L.check(rc, "mae_mask_plan_keyed")
    return plan


def _gather(x, index, out_dtype):
    """x (B, Lin, D) fp32 / bf16 contiguous, index (B, Lout) int32 -> (B, Lout, D) ``out_dtype``; one launch."""
    B, Lin, D = x.shape
    Lout = index.shape[1]
    out = torch.empty(B, Lout, D, device=x.device, dtype=out_dtype)
    rc = L.lib().fv_tokens_gather(L.ptr(x), L.i32(L.dtype_code(x.dtype)), L.ptr(index), L.ptr(out), L.i32(L.dtype_code(out_dtype)),
                                  L.i32(B), L.i32(Lin), L.i32(Lout), L.i32(D), L.stream_of(x))
    L.check(rc, "tokens_gather")
    return out


def _check_rows(who, x, index):
    L.require_gpu(x, index)
    if x.dim() != 3 or x.dtype not in _DTYPES or x.shape[-1] % 4 != 0:
        raise RuntimeError(f"{who}: rows must be (B, L, D) fp32 or bf16 with D % 4 == 0, got {tuple(x.shape)} {x.dtype}")
    if index.dim() != 2 or index.dtype != torch.int32 or index.shape[0] != x.shape[0] or not index.is_contiguous():
        raise RuntimeError(f"{who}: the index must be a contiguous (B, L_out) int32 tensor, got {tuple(index.shape)} {index.dtype}")


class _GatherTokensFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, index, adjoint_index):
        ctx.save_for_backward(adjoint_index)
        ctx.x_dtype = x.dtype
        return _gather(x.contiguous(), index, x.dtype)

    @staticmethod
    def backward(ctx, dout):
        (adjoint_index,) = ctx.saved_tensors
        if dout.dtype not in _DTYPES:
            dout = dout.float()
        return _gather(dout.contiguous(), adjoint_index, ctx.x_dtype), None, None


def gather_tokens(x, index, adjoint_index):
    """``out[b, t, :] = x[b, index[b, t], :]`` (a zero row where the index is negative) in ``x``'s dtype, bit-exact.
    ``index`` (B, L_out) int32 must not pick a row twice; ``adjoint_index`` (B, L_in) int32 is its inverse -- the ``t`` with
    ``index[b, t] == l``, -1 where row ``l`` is not picked -- and makes the backward one more gather: a ``TokenPlan``'s
    (``keep_index``, ``restore_index``) and (``order_index``, ``inverse_index``), either way round, are such pairs."""
    _check_rows("gather_tokens", x, index)
    _check_rows("gather_tokens", x, adjoint_index)
    if adjoint_index.shape[1] != x.shape[1]:
        raise RuntimeError(f"gather_tokens: adjoint_index {tuple(adjoint_index.shape)} must have one entry per row of x "
                           f"{tuple(x.shape)}")
    return _GatherTokensFn.apply(x, index, adjoint_index)


def decoder_tokens_ok(x, mask_token, pos_embed, plan):
    """Whether ``decoder_tokens`` takes these tensors (the model's fallback is the eager chain)."""
    if x.dim() != 3 or not x.is_cuda or x.dtype not in _DTYPES or x.shape[-1] % 4 != 0:
        return False
    B, K, D = x.shape
    Ln = plan.restore_index.shape[1]
    if tuple(plan.restore_index.shape) != (B, Ln) or plan.keep_index.shape[1] != K or plan.restore_index.device != x.device:
        return False
    return (mask_token.dtype == torch.float32 and mask_token.numel() == D and mask_token.is_contiguous()
            and pos_embed.dtype == torch.float32 and pos_embed.numel() == Ln * D and pos_embed.is_contiguous()
            and mask_token.device == x.device and pos_embed.device == x.device and not pos_embed.requires_grad)


class _DecoderTokensFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask_token, pos_embed, restore_index):
        B, K, D = x.shape
        Ln = restore_index.shape[1]
        xc = x.contiguous()
        out = torch.empty(B, Ln, D, device=x.device, dtype=torch.float32)
        rc = L.lib().fv_mae_decoder_tokens_fwd(L.ptr(xc), L.i32(L.dtype_code(xc.dtype)), L.ptr(mask_token), L.ptr(pos_embed),
                                               L.ptr(restore_index), L.ptr(out), L.i32(B), L.i32(Ln), L.i32(K), L.i32(D),
                                               L.stream_of(xc))
        L.check(rc, "mae_decoder_tokens_fwd")
        ctx.save_for_backward(restore_index)
        ctx.geo = (B, Ln, K, D, x.dtype, tuple(mask_token.shape))
        return out

    @staticmethod
    def backward(ctx, dout):
        (restore_index,) = ctx.saved_tensors
        B, Ln, K, D, x_dtype, mt_shape = ctx.geo
        dout = dout.float().contiguous()
        dx = torch.empty(B, K, D, device=dout.device, dtype=x_dtype)
        nblocks = -(-(B * Ln) // DECODER_ROWS_PER_BLOCK)
        partials = torch.empty(nblocks, D, device=dout.device, dtype=torch.float64)
        dmt = torch.empty(D, device=dout.device, dtype=torch.float32)
        rc = L.lib().fv_mae_decoder_tokens_bwd(L.ptr(dout), L.ptr(restore_index), L.ptr(dx), L.i32(L.dtype_code(x_dtype)),
                                               L.ptr(partials), L.i32(nblocks), L.ptr(dmt), L.i32(B), L.i32(Ln), L.i32(K),
                                               L.i32(D), L.stream_of(dout))
        L.check(rc, "mae_decoder_tokens_bwd")
        return dx, dmt.view(mt_shape), None, None


def decoder_tokens(x, mask_token, pos_embed, plan):
    """The MAE decoder's input from one launch: ``x`` (B, K, D) fp32 or bf16, the kept tokens after ``decoder_embed``;
    ``mask_token`` (1, 1, D) fp32; ``pos_embed`` (1, L, D) fp32, no gradient; ``plan`` a ``TokenPlan`` of the same step ->
    (B, L, D) fp32 = (kept token, or ``mask_token`` rounded to ``x``'s dtype) + ``pos_embed``: the values, dtype and single
    rounding of the eager ``repeat / cat / gather / add`` chain.  Backward: ``dx`` bit-identical to autograd's; ``d mask_token``
    the sum of the removed rows (rounded to ``x``'s dtype first, as autograd rounds them) in fp64 in a fixed order."""
    if not decoder_tokens_ok(x, mask_token, pos_embed, plan):
        raise RuntimeError(f"decoder_tokens: unsupported arguments (x {tuple(x.shape)} {x.dtype}, mask_token "
                           f"{tuple(mask_token.shape)} {mask_token.dtype}, pos_embed {tuple(pos_embed.shape)} {pos_embed.dtype}); "
                           "see decoder_tokens_ok")
    return _DecoderTokensFn.apply(x, mask_token, pos_embed, plan.restore_index)


# ---------------------------------------------------------------------------------------------- with a class token
def _cls_common_ok(x, vec, pos_embed, plan, Ln, K, D):
    """The part both class-token predicates share: ``vec`` (``cls_token`` / ``mask_token``) D fp32 values, ``pos_embed`` the
    whole (1, L + 1, D) fp32 table without a gradient, the plan that of x's batch, everything on x's device."""
    B = x.shape[0]
    if tuple(plan.restore_index.shape) != (B, Ln) or tuple(plan.keep_index.shape) != (B, K):
        return False
    if plan.restore_index.device != x.device or plan.keep_index.device != x.device:
        return False
    return (vec.dtype == torch.float32 and vec.numel() == D and vec.is_contiguous() and vec.device == x.device
            and pos_embed.dtype == torch.float32 and pos_embed.numel() == (Ln + 1) * D and pos_embed.is_contiguous()
            and pos_embed.device == x.device and not pos_embed.requires_grad)


def encoder_tokens_cls_ok(x, cls_token, pos_embed, plan):
    """Whether ``encoder_tokens_cls`` takes these tensors (the model's fallback is the eager chain): ``x`` (B, L, D) fp32 or
    bf16 on the GPU with D % 4 == 0, ``cls_token`` D fp32 values, ``pos_embed`` (1, L + 1, D) fp32 that does not require grad,
    ``plan`` a ``TokenPlan`` of B samples and L tokens.  Pure Python: no GPU and no library needed to ask."""
    if x.dim() != 3 or not x.is_cuda or x.dtype not in _DTYPES or x.shape[-1] % 4 != 0:
        return False
    B, Ln, D = x.shape
    return _cls_common_ok(x, cls_token, pos_embed, plan, Ln, plan.keep_index.shape[1], D)


def decoder_tokens_cls_ok(x, mask_token, pos_embed, plan):
    """Whether ``decoder_tokens_cls`` takes these tensors: ``x`` (B, K + 1, D) -- the plan's K kept tokens and the class
    token -- otherwise as ``encoder_tokens_cls_ok``, with ``mask_token`` in the place of ``cls_token``."""
    if x.dim() != 3 or not x.is_cuda or x.dtype not in _DTYPES or x.shape[-1] % 4 != 0:
        return False
    B, K1, D = x.shape
    return _cls_common_ok(x, mask_token, pos_embed, plan, plan.restore_index.shape[1], K1 - 1, D)


class _EncoderTokensClsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cls_token, pos_embed, keep_index, restore_index):
        B, Ln, D = x.shape
        K = keep_index.shape[1]
        xc = x.contiguous()
        out = torch.empty(B, K + 1, D, device=x.device, dtype=x.dtype)
        rc = L.lib().fv_mae_encoder_tokens_cls_fwd(L.ptr(xc), L.i32(L.dtype_code(xc.dtype)), L.ptr(cls_token), L.ptr(pos_embed),
                                                   L.ptr(keep_index), L.ptr(out), L.i32(B), L.i32(Ln), L.i32(K), L.i32(D),
                                                   L.stream_of(xc))
        L.check(rc, "mae_encoder_tokens_cls_fwd")
        ctx.save_for_backward(restore_index)
        ctx.geo = (B, Ln, K, D, x.dtype, tuple(cls_token.shape))
        return out

    @staticmethod
    def backward(ctx, dout):
        (restore_index,) = ctx.saved_tensors
        B, Ln, K, D, x_dtype, ct_shape = ctx.geo
        dout = dout.to(x_dtype).contiguous()
        dx = torch.empty(B, Ln, D, device=dout.device, dtype=x_dtype)
        dct = torch.empty(D, device=dout.device, dtype=torch.float32)
        rc = L.lib().fv_mae_encoder_tokens_cls_bwd(L.ptr(dout), L.ptr(restore_index), L.ptr(dx), L.i32(L.dtype_code(x_dtype)),
                                                   L.ptr(dct), L.i32(B), L.i32(Ln), L.i32(K), L.i32(D), L.stream_of(dout))
        L.check(rc, "mae_encoder_tokens_cls_bwd")
        return dx, dct.view(ct_shape), None, None, None


def encoder_tokens_cls(x, cls_token, pos_embed, plan):
    """The Vim MAE encoder's input from one launch: ``x`` (B, L, D) fp32 or bf16, the patch embedding with its position rows
    added, NOT yet gathered; ``cls_token`` (1, 1, D) fp32; ``pos_embed`` (1, L + 1, D) fp32, no gradient (its class slot, row
    0, is what is read); ``plan`` the step's ``TokenPlan`` -> (B, K + 1, D) in ``x``'s dtype: the K kept tokens with
    ``cls_token + pos_embed[:, :1]`` (added in fp32, rounded once) at place K // 2 -- the values of the eager ``gather /
    add / expand / cast / cat`` chain.  Backward: ``dx`` (every row written, zero for the removed tokens) bit-identical to
    autograd's; ``d cls_token`` the sum of the class rows over the batch, in fp64 in the order of the samples."""
    if not encoder_tokens_cls_ok(x, cls_token, pos_embed, plan):
        raise RuntimeError(f"encoder_tokens_cls: unsupported arguments (x {tuple(x.shape)} {x.dtype}, cls_token "
                           f"{tuple(cls_token.shape)} {cls_token.dtype}, pos_embed {tuple(pos_embed.shape)} {pos_embed.dtype}); "
                           "see encoder_tokens_cls_ok")
    return _EncoderTokensClsFn.apply(x, cls_token, pos_embed, plan.keep_index, plan.restore_index)


class _DecoderTokensClsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask_token, pos_embed, restore_index):
        B, K1, D = x.shape
        Ln = restore_index.shape[1]
        xc = x.contiguous()
        out = torch.empty(B, Ln + 1, D, device=x.device, dtype=torch.float32)
        rc = L.lib().fv_mae_decoder_tokens_cls_fwd(L.ptr(xc), L.i32(L.dtype_code(xc.dtype)), L.ptr(mask_token), L.ptr(pos_embed),
                                                   L.ptr(restore_index), L.ptr(out), L.i32(B), L.i32(Ln), L.i32(K1 - 1), L.i32(D),
                                                   L.stream_of(xc))
        L.check(rc, "mae_decoder_tokens_cls_fwd")
        ctx.save_for_backward(restore_index)
        ctx.geo = (B, Ln, K1 - 1, D, x.dtype, tuple(mask_token.shape))
        return out

    @staticmethod
    def backward(ctx, dout):
        (restore_index,) = ctx.saved_tensors
        B, Ln, K, D, x_dtype, mt_shape = ctx.geo
        dout = dout.float().contiguous()
        dx = torch.empty(B, K + 1, D, device=dout.device, dtype=x_dtype)
        nblocks = -(-(B * (Ln + 1)) // DECODER_ROWS_PER_BLOCK)
        partials = torch.empty(nblocks, D, device=dout.device, dtype=torch.float64)
        dmt = torch.empty(D, device=dout.device, dtype=torch.float32)
        rc = L.lib().fv_mae_decoder_tokens_cls_bwd(L.ptr(dout), L.ptr(restore_index), L.ptr(dx), L.i32(L.dtype_code(x_dtype)),
                                                   L.ptr(partials), L.i32(nblocks), L.ptr(dmt), L.i32(B), L.i32(Ln), L.i32(K),
                                                   L.i32(D), L.stream_of(dout))
        L.check(rc, "mae_decoder_tokens_cls_bwd")
        return dx, dmt.view(mt_shape), None, None


def decoder_tokens_cls(x, mask_token, pos_embed, plan):
    """The Vim MAE decoder's input from one launch: ``x`` (B, K + 1, D) fp32 or bf16, ``decoder_embed`` of the encoder's
    output (class token at place K // 2); ``mask_token`` (1, 1, D) fp32; ``pos_embed`` (1, L + 1, D) fp32, no gradient;
    ``plan`` the step's ``TokenPlan`` -> (B, L + 1, D) fp32: rows 0 .. L-1 as ``decoder_tokens`` makes them from the tokens
    without the class token and ``pos_embed[:, 1:]``, row L the class token + ``pos_embed[:, :1]`` -- the values, dtype and
    single rounding of the eager ``cat / repeat / cat / gather / add / add / cat`` chain.  Backward as ``decoder_tokens``;
    the class row is no mask row."""
    if not decoder_tokens_cls_ok(x, mask_token, pos_embed, plan):
        raise RuntimeError(f"decoder_tokens_cls: unsupported arguments (x {tuple(x.shape)} {x.dtype}, mask_token "
                           f"{tuple(mask_token.shape)} {mask_token.dtype}, pos_embed {tuple(pos_embed.shape)} {pos_embed.dtype}); "
                           "see decoder_tokens_cls_ok")
    return _DecoderTokensClsFn.apply(x, mask_token, pos_embed, plan.restore_index)
