"""Pure-torch restatement of the two chains of ``fastvim_amd.vim.VisionMamba.forward_features`` that
``fastvim_amd.vim_tokens`` replaces -- copied from it as it stands -- and of their backward, with the TERMS of the sums that
autograd adds in an order of its own.  B samples, M patch tokens, class position p.  Runs on any device."""
import torch


# ------------------------------------------------------------------------------------------------ class token + pos_embed
def cls_chain(x, cls_token, pos_embed, token_position):
    """forward_features: ``expand / to / cat`` then ``x + self.pos_embed``.  (``p = 0`` is ``torch.cat((cls_token, x), dim=1)``:
    the first slice is empty.)"""
    B = x.shape[0]
    cls_token = cls_token.expand(B, -1, -1).to(x.dtype)
    x = torch.cat((x[:, :token_position, :], cls_token, x[:, token_position:, :]), dim=1)
    return x + pos_embed


def cls_bwd(dout, token_position, x_dtype):
    """dout (B, M + 1, D) in the chain's output dtype -> (dy (B, M, D) ``x_dtype``; the B terms (B, M + 1, D) fp64 of
    d pos_embed; the B terms (B, D) fp64 of d cls_token -- rounded to ``x_dtype`` first, as the gradient of the cat is)."""
    p = token_position
    g = dout.to(x_dtype)                                            # what reaches the cat
    dy = torch.cat((g[:, :p], g[:, p + 1:]), dim=1)
    return dy, dout.double(), g[:, p].double()


# ------------------------------------------------------------------------------------------------ final norm + select
def final_chain(norm_fn, hidden_states, residual, weight, bias, eps, token_position, row_scale, is_rms_norm,
                residual_in_fp32=True):
    """forward_features with ``fused_add_norm`` and ``if_cls_token``: the norm of every row, then the class row.  ``norm_fn``
    is ``fastvim_amd.layernorm.layer_norm_fn`` (or a stand-in with its signature)."""
    hidden_states = norm_fn(hidden_states, weight, bias, eps=eps, residual=residual, prenorm=False,
                            residual_in_fp32=residual_in_fp32, is_rms_norm=is_rms_norm, row_scale=row_scale)
    return hidden_states[:, token_position, :]


def final_dout(dy_row, rows, token_position):
    """What the select hands the norm's backward: (B, rows, D), zero outside the class row."""
    B, D = dy_row.shape
    dout = torch.zeros(B, rows, D, device=dy_row.device, dtype=dy_row.dtype)
    dout[:, token_position] = dy_row
    return dout


def torch_norm(x, weight, bias, eps, residual=None, prenorm=False, residual_in_fp32=False, is_rms_norm=False, row_scale=None):
    """A plain-torch stand-in for ``layer_norm_fn`` (fp32 arithmetic, ``x``'s dtype out), for the CPU test of the wiring."""
    v = x.float()
    if row_scale is not None:
        v = v * row_scale.float().view(-1, 1, 1)
    if residual is not None:
        v = v + residual.float()
    mu = 0.0 if is_rms_norm else v.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((v - mu) ** 2).mean(-1, keepdim=True) + eps)
    out = (v - mu) * rstd * weight.float()
    if bias is not None:
        out = out + bias.float()
    return out.to(x.dtype)
