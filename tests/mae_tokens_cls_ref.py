"""Pure-torch restatement of the Vim MAE's token assembly with its class token (csrc/mae_tokens_cls.hip,
fastvim_amd/mae_tokens.py: ``encoder_tokens_cls``, ``decoder_tokens_cls``) -- the four maps as index arithmetic on the plan's
int32 indices -- and, next to it, the literal ``cat / gather / add`` chains of fastvim_amd/fastvim_mae.py that the maps stand
for.  B samples, L grid tokens, K kept, class place c = K // 2 in the encoder, L in the decoder.  Runs on any device."""
import torch


def _kept(restore_index, K):
    r = restore_index.long()
    return r, (r >= 0) & (r < K)


# ------------------------------------------------------------------------------------------------ the four maps
def encoder_fwd(x, cls_token, pos_embed, keep_index):
    """x (B, L, D), cls_token (1, 1, D) fp32, pos_embed (1, L + 1, D) fp32, keep_index (B, K) -> (B, K + 1, D) in x's dtype."""
    B, L, D = x.shape
    K = keep_index.shape[1]
    c = K // 2
    j = torch.arange(K + 1, device=x.device)
    src = torch.where(j < c, j, j - 1).clamp_min(0)                 # out row j reads keep[:, j] (j < c) or keep[:, j - 1] (j > c)
    rows = keep_index.long()[:, src]
    out = torch.gather(x, 1, rows.unsqueeze(-1).expand(-1, -1, D)).clone()
    out[:, c] = (cls_token.reshape(D).float() + pos_embed.reshape(L + 1, D)[0]).to(x.dtype)       # fp32 add, one rounding
    return out


def encoder_bwd(dout, restore_index, K):
    """dout (B, K + 1, D), restore_index (B, L) -> (dx (B, L, D) in dout's dtype, the B terms (B, D) fp64 of d cls_token)."""
    D = dout.shape[-1]
    c = K // 2
    r, kept = _kept(restore_index, K)
    j = torch.where(kept, r + (r >= c).long(), torch.zeros_like(r))
    dx = torch.gather(dout, 1, j.unsqueeze(-1).expand(-1, -1, D))
    dx = torch.where(kept.unsqueeze(-1), dx, torch.zeros_like(dx))
    return dx, dout[:, c].double()


def decoder_fwd(x, mask_token, pos_embed, restore_index):
    """x (B, K + 1, D), mask_token (1, 1, D) fp32, pos_embed (1, L + 1, D) fp32, restore_index (B, L) -> (B, L + 1, D) fp32."""
    B, K1, D = x.shape
    K, c = K1 - 1, (K1 - 1) // 2
    r, kept = _kept(restore_index, K)
    j = torch.where(kept, r + (r >= c).long(), torch.zeros_like(r))
    rows = torch.gather(x, 1, j.unsqueeze(-1).expand(-1, -1, D))
    body = torch.where(kept.unsqueeze(-1), rows, mask_token.reshape(1, 1, D).to(x.dtype)) + pos_embed[:, 1:]
    last = x[:, c:c + 1] + pos_embed[:, :1]
    return torch.cat([body.float(), last.float()], dim=1)


def decoder_bwd(dout, keep_index, restore_index, x_dtype):
    """dout (B, L + 1, D) fp32 -> (dx (B, K + 1, D) ``x_dtype``, the terms (n_removed, D) fp64 of d mask_token: the removed
    rows, rounded to ``x_dtype`` first; the class row L of a sample is no mask row)."""
    B, L1, D = dout.shape
    L, K = L1 - 1, keep_index.shape[1]
    c = K // 2
    j = torch.arange(K + 1, device=dout.device)
    src = torch.where(j < c, j, j - 1).clamp_min(0)
    rows = keep_index.long()[:, src]
    rows[:, c] = L                                                  # row c takes dout[b, L]
    dx = torch.gather(dout, 1, rows.unsqueeze(-1).expand(-1, -1, D)).to(x_dtype)
    _, kept = _kept(restore_index, K)
    return dx, dout[:, :L][~kept].to(x_dtype).double()


# ------------------------------------------------------------------------------------------------ the chains, as written
def encoder_chain(x, cls_token, pos_embed, ids_keep):
    """fastvim_mae.py:97-102 behind the masking gather of ``random_masking``."""
    x = torch.gather(x, dim=1, index=ids_keep.unsqueeze(-1).repeat(1, 1, x.shape[2]))
    M = x.shape[1]
    cls_tokens = (cls_token + pos_embed[:, :1, :]).expand(x.shape[0], -1, -1).to(x.dtype)
    token_position = M // 2
    return torch.cat((x[:, :token_position, :], cls_tokens, x[:, token_position:, :]), dim=1)


def decoder_chain(x, mask_token, decoder_pos_embed, ids_restore):
    """fastvim_mae.py:117-125 behind ``decoder_embed``."""
    token_position = (x.shape[1] - 1) // 2
    mask_tokens = mask_token.repeat(x.shape[0], ids_restore.shape[1] + 1 - x.shape[1], 1).to(x.dtype)
    x_ = torch.cat([x[:, :token_position, :], x[:, token_position + 1:, :], mask_tokens], dim=1)
    x_ = torch.gather(x_, dim=1, index=ids_restore.unsqueeze(-1).repeat(1, 1, x.shape[2]))
    x_ = x_ + decoder_pos_embed[:, 1:]
    cls_tokens = x[:, token_position:token_position + 1, :] + decoder_pos_embed[:, :1, :]
    return torch.cat([x_, cls_tokens.to(x_.dtype)], dim=1)


def sum_bound(terms):
    """The project's criterion for a sum accumulated in fp64 and rounded once to fp32 (``mask_token_bound`` of
    tests/test_mae_tokens_gpu.py with c_adds = 0): |err| <= 2^-24 sum|terms| per channel; ``terms`` (n, D) fp64."""
    return 2.0 ** -24 * terms.abs().sum(0)
