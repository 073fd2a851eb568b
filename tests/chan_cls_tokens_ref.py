"""Pure-torch restatement of the two launches of csrc/chan_tokens.hip (``fastvim_amd.chan_tokens``) as index arithmetic, and,
next to it, the chain of ``fastvim_amd.models_channel_mamba.VisionMamba.forward_features`` that they stand for -- copied from
it as it stands.  B samples, M channel tokens, class position p (0 <= p <= M).  Runs on any device."""
import torch


def fwd(y, cls_token, p):
    """y (B, M, D) in T, cls_token (1, 1, D) fp32 -> (B, M + 1, D) in T: row j is cls_token rounded to T when j == p, else
    y[:, j - (j > p)] (the bits move: an index_select)."""
    B, M, D = y.shape
    j = torch.arange(M + 1, device=y.device)
    src = (j - (j > p).long()).clamp(0, M - 1)
    out = y.index_select(1, src).clone()
    out[:, p] = cls_token.reshape(D).to(y.dtype)
    return out


def bwd(dout, p):
    """dout (B, M + 1, D) in T -> (dy (B, M, D) in T: dy[:, i] = dout[:, i + (i >= p)], the bits; the B terms (B, D) fp64 of
    d cls_token: dout[:, p])."""
    M = dout.shape[1] - 1
    i = torch.arange(M, device=dout.device)
    return dout.index_select(1, i + (i >= p).long()), dout[:, p].double()


def chain(x, cls_token, token_position):
    """forward_features: ``expand / to / cat``."""
    B = x.shape[0]
    cls_token = cls_token.expand(B, -1, -1).to(x.dtype)
    return torch.cat((x[:, :token_position, :], cls_token, x[:, token_position:, :]), dim=1)
