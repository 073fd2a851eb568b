"""The restatement of the Vim baseline's class-token chains (tests/vim_tokens_ref.py) against
``fastvim_amd.vim.VisionMamba.forward_features`` itself, on the CPU -- the patch projection and the norm, which have no CPU
form, are stood in for; everything between them is the model's own code -- its backward against autograd, and the
pure-Python predicates of ``fastvim_amd.vim_tokens``.  No GPU and no library needed."""
import pytest
import torch

import mae_tokens_cls_ref as C
import vim_tokens_ref as V

B, SIZE, D = 3, 64, 8          # 4 x 4 grid: M = 16
M = 16


def _model(middle):
    from fastvim_amd.vim import VisionMamba
    torch.manual_seed(5)
    return VisionMamba(img_size=SIZE, patch_size=16, depth=0, embed_dim=D, num_classes=4, rms_norm=True, residual_in_fp32=True,
                       fused_add_norm=True, drop_path_rate=0.0, use_middle_cls_token=middle)


@pytest.mark.parametrize("middle", [True, False], ids=["p=M//2", "p=0"])
@pytest.mark.parametrize("fused_cls", [False, True], ids=["chain", "fused_cls"])
def test_restatement_equals_forward_features(middle, fused_cls, monkeypatch):
    """``fused_cls`` on a CPU model: both predicates say no, so ``_embed`` / ``_final`` run the torch chains -- the same
    values through the other entry."""
    import fastvim_amd.vim as vim
    m = _model(middle)
    m.fused_cls = fused_cls
    p = M // 2 if middle else 0
    g = torch.Generator().manual_seed(1)
    y = torch.randn(B, M, D, generator=g)
    with torch.no_grad():
        m.pos_embed.copy_(torch.randn(1, M + 1, D, generator=g))
        m.cls_token.copy_(torch.randn(1, 1, D, generator=g))
        m.norm_f.weight.copy_(torch.rand(D, generator=g) + 0.5)
    monkeypatch.setattr(type(m.patch_embed), "forward", lambda self, x, **kw: y)
    monkeypatch.setattr(vim, "layer_norm_fn", V.torch_norm)
    got = m.forward_features(torch.zeros(B, 3, SIZE, SIZE))
    tokens = V.cls_chain(y, m.cls_token, m.pos_embed, p)
    assert tokens.shape == (B, M + 1, D)
    assert torch.equal(tokens[:, p], (m.cls_token + m.pos_embed[:, p]).expand(B, 1, D)[:, 0])
    want = V.final_chain(V.torch_norm, tokens, None, m.norm_f.weight, None, m.norm_f.eps, p, None, True)
    assert got.shape == (B, D) and torch.equal(got, want)
    if fused_cls:
        h, (Hg, Wg) = m._embed(torch.zeros(B, 3, SIZE, SIZE))
        assert (Hg, Wg) == (4, 4) and torch.equal(h, tokens)
        assert torch.equal(m._final(h, None), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("p", [0, 4, 9])
def test_restated_backward_equals_autograd(p, dtype):
    g = torch.Generator().manual_seed(10 + p)
    Mo = 9
    y = torch.randn(B, Mo, D, generator=g).to(dtype).requires_grad_(True)
    cls = (0.02 * torch.randn(1, 1, D, generator=g)).requires_grad_(True)
    pos = torch.randn(1, Mo + 1, D, generator=g).requires_grad_(True)
    out = V.cls_chain(y, cls, pos, p)
    assert out.dtype == torch.float32                      # a bf16 y promotes against the fp32 table
    dout = torch.randn(B, Mo + 1, D, generator=g)
    out.backward(dout)
    dy, pos_terms, cls_terms = V.cls_bwd(dout, p, dtype)
    assert dy.dtype == y.grad.dtype == dtype and torch.equal(dy, y.grad)
    # autograd adds B terms in fp32 (bf16 for the class token of a bf16 y) in some order
    err = (pos.grad.double() - pos_terms.sum(0)).abs().view(-1, D)
    assert bool((err <= B * C.sum_bound(pos_terms.view(B, -1)).view(-1, D)).all())
    ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -24
    err = (cls.grad.double().view(D) - cls_terms.sum(0)).abs()
    assert bool((err <= B * ulp * cls_terms.abs().sum(0)).all())


# ------------------------------------------------------------------------------------------------ predicates
class _OnGpu(torch.Tensor):
    """A CPU tensor that answers ``is_cuda`` with True: the predicates are pure Python, so everything behind their first
    question can be asked without a GPU."""
    is_cuda = property(lambda self: True)


def _gpu(t):
    return t.as_subclass(_OnGpu)


def test_cls_tokens_predicate():
    from fastvim_amd import vim_tokens as T
    y, cls, pos = torch.zeros(2, 16, 32), torch.zeros(1, 1, 32), torch.zeros(1, 17, 32)
    assert not T.cls_tokens_ok(y, cls, pos, 8)                                   # a CPU tensor
    assert T.cls_tokens_ok(_gpu(y), cls, pos, 8) and T.cls_tokens_ok(_gpu(y.bfloat16()), cls, pos, 0)
    assert T.cls_tokens_ok(_gpu(y), cls, pos, 16) and not T.cls_tokens_ok(_gpu(y), cls, pos, 17)
    assert not T.cls_tokens_ok(_gpu(y), cls, pos, -1)
    assert not T.cls_tokens_ok(_gpu(y.half()), cls, pos, 8)
    assert not T.cls_tokens_ok(_gpu(torch.zeros(2, 32, 16).transpose(1, 2)), cls, pos, 8)      # not contiguous
    assert not T.cls_tokens_ok(_gpu(torch.zeros(2, 16, 30)), torch.zeros(1, 1, 30), torch.zeros(1, 17, 30), 8)
    assert T.cls_tokens_ok(_gpu(torch.zeros(2, 16, 36)), torch.zeros(1, 1, 36), torch.zeros(1, 17, 36), 8)
    assert not T.cls_tokens_ok(_gpu(y), cls.bfloat16(), pos, 8) and not T.cls_tokens_ok(_gpu(y), cls, pos[:, :16], 8)
    with pytest.raises(RuntimeError, match="cls_tokens_ok"):
        T.cls_tokens(y, cls, pos, 8)


def test_add_norm_row_predicate():
    from fastvim_amd import vim_tokens as T
    h, r, w = torch.zeros(2, 17, 32), torch.zeros(2, 17, 32), torch.ones(32)
    assert not T.add_norm_row_ok(h, r, w, None, 8)                               # a CPU tensor
    assert T.add_norm_row_ok(_gpu(h), r, w, None, 8) and T.add_norm_row_ok(_gpu(h.bfloat16()), r, w, w, 16, torch.ones(2))
    assert not T.add_norm_row_ok(_gpu(h), r, w, None, 17)
    assert not T.add_norm_row_ok(_gpu(h), r, w, None, 8, None, False)            # residual_in_fp32 is part of the predicate
    assert not T.add_norm_row_ok(_gpu(h), None, w, None, 8) and not T.add_norm_row_ok(_gpu(h), r.bfloat16(), w, None, 8)
    assert not T.add_norm_row_ok(_gpu(h.half()), r, w, None, 8)
    assert not T.add_norm_row_ok(_gpu(torch.zeros(2, 17, 30)), torch.zeros(2, 17, 30), torch.ones(30), None, 8)
    assert not T.add_norm_row_ok(_gpu(torch.zeros(2, 17, 2052)), torch.zeros(2, 17, 2052), torch.ones(2052), None, 8)
    assert not T.add_norm_row_ok(_gpu(torch.zeros(2, 32, 17).transpose(1, 2)), torch.zeros(2, 17, 32), w, None, 8)
    assert not T.add_norm_row_ok(_gpu(h), r, w, None, 8, torch.ones(3))
    with pytest.raises(RuntimeError, match="add_norm_row_ok"):
        T.add_norm_row(h, r, w, None, 1e-5, 8)
