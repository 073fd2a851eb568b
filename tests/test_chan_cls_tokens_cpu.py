"""The restatement of the ChannelVim class-token launches (tests/chan_cls_tokens_ref.py) against the torch chain of
``fastvim_amd.models_channel_mamba.VisionMamba.forward_features`` and its autograd, on the CPU; the model's segment methods
with the patch projection and the norm -- which have no CPU form -- stood in for; and the pure-Python predicate of
``fastvim_amd.chan_tokens``.  No GPU and no library needed."""
import pytest
import torch

import chan_cls_tokens_ref as R
import vim_tokens_ref as V
from mae_tokens_cls_ref import sum_bound

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
SHAPES = [(B, M, D) for B in (1, 3) for M in (1, 2, 7, 12) for D in (4, 36)]


def _inputs(B, M, D, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + B * 1000 + M * 50 + D)
    y = torch.randn(B, M, D, generator=g).to(dtype)
    y.view(-1)[0] = -0.0                                     # a sign that an added zero would lose
    cls = 0.02 * torch.randn(1, 1, D, generator=g)
    dout = torch.randn(B, M + 1, D, generator=g).to(dtype)
    return y, cls, dout


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,M,D", SHAPES)
def test_restatement_equals_the_chain_and_its_autograd(B, M, D, dtype):
    for p in sorted({0, M // 2, M}):
        y, cls, dout = _inputs(B, M, D, dtype, p)
        ya, ca = y.clone().requires_grad_(True), cls.clone().requires_grad_(True)
        want = R.chain(ya, ca, p)
        got = R.fwd(y, cls, p)
        assert got.dtype == want.dtype == dtype and got.shape == (B, M + 1, D)
        assert torch.equal(got.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                           want.detach().view(torch.int16 if dtype == torch.bfloat16 else torch.int32))      # the bits
        assert torch.equal(got[:, p], cls.to(dtype).expand(B, 1, D)[:, 0])
        want.backward(dout)
        dy, terms = R.bwd(dout, p)
        assert dy.dtype == dtype and dy.shape == (B, M, D) and torch.equal(dy, ya.grad)
        assert terms.shape == (B, D) and terms.dtype == torch.float64
        exact = terms.sum(0)
        # the launch's sum: fp64 in the order of the samples, one rounding
        acc = torch.zeros(D, dtype=torch.float64)
        for b in range(B):
            acc = acc + terms[b]
        assert bool(((acc.float().double() - exact).abs() <= sum_bound(terms)).all())
        # autograd adds the B terms in fp32 in an order of its own: at most B roundings
        assert ca.grad.dtype == torch.float32
        assert bool(((ca.grad.double().view(D) - exact).abs() <= B * sum_bound(terms)).all())


def _model(fused_cls):
    from fastvim_amd.models_channel_mamba import VisionMamba
    torch.manual_seed(5)
    return VisionMamba(img_size=32, patch_size=16, depth=0, embed_dim=8, channels=3, num_classes=4, rms_norm=True,
                       residual_in_fp32=True, fused_add_norm=True, if_cls_token=True, if_abs_pos_embed=True, drop_path_rate=0.0,
                       fused_cls=fused_cls)


@pytest.mark.parametrize("n_chan", [3, 2, 1])
@pytest.mark.parametrize("fused_cls", [False, True], ids=["chain", "fused_cls"])
def test_segment_methods_equal_forward_features(fused_cls, n_chan, monkeypatch):
    """On a CPU model the predicates say no, so ``fused_cls`` runs the torch chains through ``_embed`` / ``_final``: the
    values of the monolithic ``forward_features``, with the class position following the channel count."""
    import fastvim_amd.models_channel_mamba as cm
    m = _model(fused_cls)
    assert m.fused_cls is fused_cls and _model(False).fused_cls is False
    B, P, D = 2, 4, 8
    M = P * n_chan
    g = torch.Generator().manual_seed(n_chan)
    y = torch.randn(B, M, D, generator=g)
    seen = {}

    def embed(self, x, pos_embed=None, hcs=None, **kw):
        seen["pos"], seen["hcs"] = pos_embed, hcs
        return y, n_chan, 32, 32, list(range(n_chan))
    with torch.no_grad():
        m.cls_token.copy_(torch.randn(1, 1, D, generator=g))
        m.norm_f.weight.copy_(torch.rand(D, generator=g) + 0.5)
    monkeypatch.setattr(type(m.patch_embed), "forward", embed)
    monkeypatch.setattr(cm, "layer_norm_fn", V.torch_norm)
    x = torch.zeros(B, 3, 32, 32)
    p = M // 2
    tokens = R.chain(y, m.cls_token, p)
    want = V.final_chain(V.torch_norm, tokens, None, m.norm_f.weight, None, m.norm_f.eps, p, None, True)
    got = m.forward_features(x)
    assert got.shape == (B, D) and torch.equal(got, want)
    assert seen["pos"] is m.pos_embed and seen["hcs"] is None
    sampler = object()
    assert torch.equal(m.forward_features(x, hcs=sampler), want) and seen["hcs"] is sampler      # eager mode takes it too
    h, (hh, ww) = m._embed(x, hcs=sampler)
    assert (hh, ww) == (32, 32) and torch.equal(h, tokens) and torch.equal(h, R.fwd(y, m.cls_token, p))
    h, res = m._run_layers(h, None, 0, 0)
    assert res is None and torch.equal(m._final(h, res), want)
    assert torch.equal(m._head(want), torch.nn.functional.linear(want, m.head.weight, m.head.bias))
    assert torch.equal(m(x, hcs=sampler), m(x))


# ------------------------------------------------------------------------------------------------ predicate
class _OnGpu(torch.Tensor):
    """A CPU tensor that answers ``is_cuda`` with True: the predicate is pure Python, so everything behind its first
    question can be asked without a GPU."""
    is_cuda = property(lambda self: True)


def _gpu(t):
    return t.as_subclass(_OnGpu)


def test_chan_cls_tokens_predicate():
    from fastvim_amd import chan_tokens as T
    y, cls = torch.zeros(2, 12, 32), torch.zeros(1, 1, 32)
    assert not T.chan_cls_tokens_ok(y, cls, 6)                                   # a CPU tensor
    assert T.chan_cls_tokens_ok(_gpu(y), cls, 6) and T.chan_cls_tokens_ok(_gpu(y.bfloat16()), cls, 0)
    assert T.chan_cls_tokens_ok(_gpu(y), cls, 12) and not T.chan_cls_tokens_ok(_gpu(y), cls, 13)
    assert not T.chan_cls_tokens_ok(_gpu(y), cls, -1) and not T.chan_cls_tokens_ok(_gpu(y), cls, 6.0)
    assert not T.chan_cls_tokens_ok(_gpu(y), cls, True)
    assert not T.chan_cls_tokens_ok(_gpu(y.half()), cls, 6) and not T.chan_cls_tokens_ok(_gpu(y.double()), cls.double(), 6)
    assert not T.chan_cls_tokens_ok(_gpu(torch.zeros(2, 32, 12).transpose(1, 2)), cls, 6)      # not contiguous
    assert not T.chan_cls_tokens_ok(_gpu(torch.zeros(2, 12, 30)), torch.zeros(1, 1, 30), 6)
    assert T.chan_cls_tokens_ok(_gpu(torch.zeros(2, 12, 36)), torch.zeros(1, 1, 36), 6)
    assert T.chan_cls_tokens_ok(_gpu(torch.zeros(1, 1, 4)), torch.zeros(4), 1)
    assert not T.chan_cls_tokens_ok(_gpu(y), cls.bfloat16(), 6) and not T.chan_cls_tokens_ok(_gpu(y), torch.zeros(1, 1, 16), 6)
    assert not T.chan_cls_tokens_ok(_gpu(torch.zeros(2, 12)), cls, 6) and not T.chan_cls_tokens_ok(None, cls, 6)
    assert not T.chan_cls_tokens_ok(_gpu(torch.zeros(0, 12, 32)), cls, 6)
    odd = torch.zeros(2 * 12 * 32 + 1, dtype=torch.bfloat16)[1:].view(2, 12, 32)               # 2-byte aligned only
    assert not T.chan_cls_tokens_ok(_gpu(odd), cls, 6)
    with pytest.raises(RuntimeError, match="chan_cls_tokens_ok"):
        T.chan_cls_tokens(y, cls, 6)
    # the chooser takes the chain there: the same values, and autograd's gradients
    g = torch.Generator().manual_seed(0)
    ya, ca = torch.randn(2, 12, 32, generator=g).requires_grad_(True), torch.randn(1, 1, 32, generator=g).requires_grad_(True)
    out = T.assemble(ya, ca, 6)
    assert torch.equal(out, R.fwd(ya.detach(), ca.detach(), 6)) and torch.equal(out, T.chan_cls_tokens_chain(ya, ca, 6))
    dout = torch.randn(2, 13, 32, generator=g)
    out.backward(dout)
    assert torch.equal(ya.grad, R.bwd(dout, 6)[0])
