"""The class token of the ChannelVim baseline on the HIP path (``fastvim_amd.models_channel_mamba.VisionMamba.fused_cls``).

``chan_cls_tokens`` (csrc/chan_tokens.hip) puts the class token among the channel tokens: one launch where
``forward_features`` runs ``expand / to / cat`` -- and one launch backward where autograd runs two slice copies, a cat and a
sum over the batch.  ``pos_embed`` has no class slot in this model and is already inside the tokens (the channel patch
projection's epilogue adds it), so nothing is added here: the token rows are moved bit for bit, in the tokens' own dtype, and
the backward is a parallel copy with the class row's sum as a few threads of the same launch.  (``vim_tokens.cls_tokens``
always adds a table and writes fp32: a zero table would turn ``-0.0`` into ``+0.0``, and its fused ``d pos_embed`` sum makes
its backward a walk over the batch.)  The model's tail is ``vim_tokens.add_norm_row`` as it stands.

Values equal the torch chain bit for bit.  What differs is the order of one sum -- ``cls_token.grad``, here in fp64 in the
order of the samples, rounded once.

``chan_cls_tokens_ok`` is pure Python: no GPU and no library needed to ask.  The op raises where the predicate says no;
``assemble`` and the model choose the torch chain there.  Nothing here synchronises with the host; outputs are allocated by
torch on the current stream: safe under graph capture.
"""
import torch

from . import _lib as L

_DTYPES = (torch.float32, torch.bfloat16)


def chan_cls_tokens_ok(y, cls_token, position):
    """Whether ``chan_cls_tokens`` takes these arguments: ``y`` (B, M, D) fp32 or bf16, contiguous, on the GPU, 4-byte
    aligned, D % 4 == 0, B (M + 1) < 2^31; ``cls_token`` D fp32 values, contiguous, on y's device; 0 <= position <= M."""
    if not isinstance(y, torch.Tensor) or y.dim() != 3 or not y.is_cuda or y.dtype not in _DTYPES or not y.is_contiguous():
        return False
    B, M, D = y.shape
    if B <= 0 or M <= 0 or D <= 0 or D % 4 != 0 or B * (M + 1) >= 2 ** 31 or B * (M + 1) * (D // 4) > 2 ** 38:
        return False
    if y.storage_offset() * y.element_size() % 4 != 0:
        return False
    if not (isinstance(cls_token, torch.Tensor) and cls_token.dtype == torch.float32 and cls_token.numel() == D
            and cls_token.is_contiguous() and cls_token.device == y.device):
        return False
    return isinstance(position, int) and not isinstance(position, bool) and 0 <= position <= M


def chan_cls_tokens_chain(y, cls_token, position):
    """The torch chain of ``forward_features`` that ``chan_cls_tokens`` stands for."""
    cls = cls_token.expand(y.shape[0], -1, -1).to(y.dtype)
    return torch.cat((y[:, :position, :], cls, y[:, position:, :]), dim=1)


class _ChanClsTokensFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, cls_token, position):
        B, M, D = y.shape
        out = torch.empty(B, M + 1, D, device=y.device, dtype=y.dtype)
        rc = L.lib().fv_chan_cls_tokens_fwd(L.ptr(y), L.i32(L.dtype_code(y.dtype)), L.ptr(cls_token), L.ptr(out), L.i32(B),
                                            L.i32(M), L.i32(D), L.i32(position), L.stream_of(y))
        L.check(rc, "chan_cls_tokens_fwd")
        ctx.geo = (B, M, D, position, y.dtype, tuple(cls_token.shape))
        return out

    @staticmethod
    def backward(ctx, dout):
        B, M, D, position, dtype, ct_shape = ctx.geo
        dout = dout.to(dtype).contiguous()
        dy = torch.empty(B, M, D, device=dout.device, dtype=dtype)
        dcls = torch.empty(D, device=dout.device, dtype=torch.float32)
        rc = L.lib().fv_chan_cls_tokens_bwd(L.ptr(dout), L.ptr(dy), L.i32(L.dtype_code(dtype)), L.ptr(dcls), L.i32(B), L.i32(M),
                                            L.i32(D), L.i32(position), L.stream_of(dout))
        L.check(rc, "chan_cls_tokens_bwd")
        return dy, dcls.view(ct_shape), None


def chan_cls_tokens(y, cls_token, position):
    """``y`` (B, M, D) fp32 or bf16, the channel tokens with ``pos_embed`` in them; ``cls_token`` (1, 1, D) fp32;
    ``position`` the class token's row -> (B, M + 1, D) in ``y``'s dtype: row j is ``cls_token.to(y.dtype)`` when
    ``j == position``, else ``y[:, j - (j > position)]`` -- the values of ``chan_cls_tokens_chain``, bit for bit (no
    arithmetic on the token rows).  Backward: ``dy`` bit-identical to autograd's; ``d cls_token`` the sum over the batch in
    fp64 in the order of the samples, rounded once to fp32."""
    if not chan_cls_tokens_ok(y, cls_token, position):
        raise RuntimeError(f"chan_cls_tokens: unsupported arguments (y {tuple(y.shape)} {y.dtype} on {y.device}, cls_token "
                           f"{tuple(cls_token.shape)} {cls_token.dtype}, position {position!r}); see chan_cls_tokens_ok")
    return _ChanClsTokensFn.apply(y, cls_token, position)


def assemble(y, cls_token, position):
    """``chan_cls_tokens`` where its predicate holds, the torch chain elsewhere: the same values either way."""
    if chan_cls_tokens_ok(y, cls_token, position):
        return _ChanClsTokensFn.apply(y, cls_token, position)
    return chan_cls_tokens_chain(y, cls_token, position)
