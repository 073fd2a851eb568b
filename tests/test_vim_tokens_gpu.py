"""``fastvim_amd.vim_tokens`` (csrc/vim_tokens.hip; the row kernels of csrc/norm.hip) against the torch chains of
``fastvim_amd.vim.VisionMamba.forward_features`` (tests/vim_tokens_ref.py): values and row gradients bit for bit, the summed
gradients within one fp32 rounding of the fp64 sum of the same terms (``cls_token`` / ``pos_embed``) and within the
``dw`` / ``db`` bounds of tests/norm_checks.py applied to the B class rows (the final norm's weight and bias)."""
import functools

import pytest
import torch

import norm_checks as NC
import vim_tokens_ref as V
from mae_tokens_cls_ref import sum_bound

pytestmark = pytest.mark.gpu

CASES = [(3, 16, 32, 8),          # base case
         (2, 9, 32, 4),           # odd M
         (2, 16, 36, 8),          # D % 8 != 0: a bf16 thread moves 4 channels
         (2, 16, 32, 0),          # class token first
         (2, 16, 32, 16),         # p = M: kernel level only, no model makes it
         (1, 196, 192, 98),       # Vim-T's 197 rows
         (2, 1024, 1280, 512)]    # the largest recipe grid at the widest model
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]


@functools.lru_cache(maxsize=None)
def _cls_inputs(B, M, D, p, dtype):
    """Inputs and the chain's results, once per case; read-only."""
    g = torch.Generator().manual_seed(B * 1000 + M + D + p)
    y = torch.randn(B, M, D, generator=g).to(dtype).cuda()
    cls = (0.02 * torch.randn(1, 1, D, generator=g)).cuda()
    pos = torch.randn(1, M + 1, D, generator=g).cuda()
    dout = torch.randn(B, M + 1, D, generator=g).cuda()
    out = V.cls_chain(y, cls, pos, p)
    dy, pos_terms, cls_terms = V.cls_bwd(dout, p, dtype)
    return y, cls, pos, dout, out, dy, pos_terms, cls_terms


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,M,D,p", CASES)
def test_cls_tokens_equals_the_chain(B, M, D, p, dtype):
    from fastvim_amd import vim_tokens as T
    y, cls, pos, dout, want, want_dy, pos_terms, cls_terms = _cls_inputs(B, M, D, p, dtype)
    runs = []
    for _ in range(2):
        ya, ca, pa = y.clone().requires_grad_(True), cls.clone().requires_grad_(True), pos.clone().requires_grad_(True)
        assert T.cls_tokens_ok(ya, ca, pa, p)
        out = T.cls_tokens(ya, ca, pa, p)
        out.backward(dout)
        runs.append((out.detach(), ya.grad, pa.grad, ca.grad))
    out, dy, dpos, dcls = runs[0]
    assert out.dtype == want.dtype == torch.float32 and out.shape == (B, M + 1, D) and torch.equal(out, want)
    assert dy.dtype == dtype and dy.shape == (B, M, D) and torch.equal(dy, want_dy)
    assert dpos.shape == pos.shape and dcls.shape == cls.shape and dpos.dtype == dcls.dtype == torch.float32
    err = (dpos.double().view(-1) - pos_terms.sum(0).view(-1)).abs()
    bound = sum_bound(pos_terms.view(B, -1))
    print(f"d pos_embed: max err {err.max().item():.3e}, max err/bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert bool((err <= bound).all())
    err = (dcls.double().view(-1) - cls_terms.sum(0)).abs()
    bound = sum_bound(cls_terms)
    print(f"d cls_token: max err {err.max().item():.3e}, max err/bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert bool((err <= bound).all())
    if dtype == torch.float32:
        assert torch.equal(dcls.view(-1), dpos.view(M + 1, D)[p])            # the same sum
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))          # a second run: the same bits


@pytest.mark.parametrize("what", ["cpu", "non_contiguous", "D=30"])
def test_cls_tokens_refusals_take_the_chain(what):
    from fastvim_amd import vim_tokens as T
    g = torch.Generator().manual_seed(3)
    B, M, D, p = 2, 16, (30 if what == "D=30" else 32), 8
    dev = "cpu" if what == "cpu" else "cuda"
    y = torch.randn(B, M, D, generator=g).to(dev)
    if what == "non_contiguous":
        y = torch.randn(B, D, M, generator=g).to(dev).transpose(1, 2)
    cls, pos = torch.randn(1, 1, D, generator=g).to(dev), torch.randn(1, M + 1, D, generator=g).to(dev)
    assert not T.cls_tokens_ok(y, cls, pos, p)
    with pytest.raises(RuntimeError, match="cls_tokens_ok"):
        T.cls_tokens(y, cls, pos, p)
    ya, ca, pa = y.clone().requires_grad_(True), cls.clone().requires_grad_(True), pos.clone().requires_grad_(True)
    out = T.assemble(ya, ca, pa, p)
    want = V.cls_chain(y, cls, pos, p)
    assert torch.equal(out, want)
    dout = torch.randn(B, M + 1, D, generator=g).to(dev)
    out.backward(dout)
    dy, pos_terms, cls_terms = V.cls_bwd(dout, p, y.dtype)
    assert torch.equal(ya.grad, dy)
    assert bool(((pa.grad.double().view(-1) - pos_terms.sum(0).view(-1)).abs() <= B * sum_bound(pos_terms.view(B, -1))).all())
    assert bool(((ca.grad.double().view(-1) - cls_terms.sum(0)).abs() <= B * sum_bound(cls_terms)).all())


# ------------------------------------------------------------------------------------------------ the tail: one row
@functools.lru_cache(maxsize=None)
def _norm_inputs(B, M, D, dtype):
    g = torch.Generator().manual_seed(B * 7 + M + D)
    T_ = M + 1
    hidden = torch.randn(B, T_, D, generator=g).to(dtype).cuda()
    residual = torch.randn(B, T_, D, generator=g).cuda()
    w = (1 + 0.1 * torch.randn(D, generator=g)).cuda()
    b = (0.1 * torch.randn(D, generator=g)).cuda()
    scale = (1.0 / (1.0 - 0.05 * (1 + torch.arange(B, dtype=torch.float32)))).cuda()
    dy = torch.randn(B, D, generator=g).to(dtype).cuda()
    return hidden, residual, w, b, scale, dy


@pytest.mark.parametrize("with_scale", [False, True], ids=["noscale", "scale"])
@pytest.mark.parametrize("rms", [True, False], ids=["rms", "ln"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,M,D,p", CASES)
def test_add_norm_row_equals_the_whole_norm(B, M, D, p, dtype, rms, with_scale):
    from fastvim_amd import vim_tokens as T
    from fastvim_amd.layernorm import layer_norm_fn
    hidden, residual, w, b, scale, dy = _norm_inputs(B, M, D, dtype)
    b = None if rms else b
    scale = scale if with_scale else None
    eps, rows = 1e-5, M + 1

    def leaves():
        return (hidden.clone().requires_grad_(True), residual.clone().requires_grad_(True), w.clone().requires_grad_(True),
                None if b is None else b.clone().requires_grad_(True))
    # the chain: the norm of every row, the class row selected; its backward is the norm's over a dout zero outside row p
    h0, r0, w0, b0 = leaves()
    want = V.final_chain(layer_norm_fn, h0, r0, w0, b0, eps, p, scale, rms)
    want.backward(dy)
    h1, r1, w1, b1 = leaves()
    assert T.add_norm_row_ok(h1, r1, w1, b1, p, scale, True)
    got = T.add_norm_row(h1, r1, w1, b1, eps, p, scale, rms, True)
    assert got.dtype == dtype and got.shape == (B, D) and torch.equal(got, want)
    got.backward(dy)
    for name, a, ref in (("d hidden", h1.grad, h0.grad), ("d residual", r1.grad, r0.grad)):
        assert a.dtype == ref.dtype and a.shape == (B, rows, D)
        assert torch.equal(a[:, p], ref[:, p]), name
        other = torch.ones(rows, dtype=torch.bool, device="cuda")
        other[p] = False
        assert not a[:, other].any() and not ref[:, other].any(), name       # exact zeros, every element
    assert r1.grad.dtype == torch.float32 and h1.grad.dtype == dtype
    # d weight / d bias: the norm_checks bounds on the B gathered rows
    ref = NC.reference(hidden[:, p], w, b, residual[:, p], scale, eps, rms, dy, None)
    msg = NC.check_dw(w1.grad, ref)
    assert not msg, msg
    if b is not None:
        msg = NC.check_db(b1.grad, ref)
        assert not msg, msg


@pytest.mark.parametrize("rms", [True, False], ids=["rms", "ln"])
@pytest.mark.parametrize("B,M,D,p", [CASES[0], CASES[5], CASES[6]])
def test_add_norm_row_backward_writes_every_element(B, M, D, p, rms):
    """The one launch into buffers pre-filled with NaN: no element survives (an unwritten row cannot hide in an ``empty``
    buffer), and the values are those of the op."""
    from fastvim_amd import vim_tokens as T
    hidden, residual, w, b, scale, dy = _norm_inputs(B, M, D, torch.bfloat16)
    b = None if rms else b
    h1, r1 = hidden.clone().requires_grad_(True), residual.clone().requires_grad_(True)
    T.add_norm_row(h1, r1, w, b, 1e-5, p, scale, rms, True).backward(dy)
    fn = T._AddNormRowFn
    ctx = type("Ctx", (), {"save_for_backward": lambda self, *t: setattr(self, "saved", t)})()
    fn.forward(ctx, hidden, residual, w, b, 1e-5, p, scale, rms)
    r, wf, bf, mean, rstd, sc = ctx.saved
    dh = torch.full((B, M + 1, D), float("nan"), device="cuda", dtype=torch.bfloat16)
    dr = torch.full((B, M + 1, D), float("nan"), device="cuda", dtype=torch.float32)
    out = T.add_norm_row_backward(dy, r, wf, mean, rstd, sc, M + 1, p, rms, torch.bfloat16, bf is not None, dhidden=dh,
                                  dresidual=dr)
    assert out[0] is dh and out[1] is dr
    assert not torch.isnan(dh).any() and not torch.isnan(dr).any()
    assert torch.equal(dh, h1.grad) and torch.equal(dr, r1.grad)


def test_add_norm_row_refusals_take_the_whole_norm():
    """A non-contiguous ``hidden`` and a bf16 residual: the predicate says no, the op raises, and the model's ``_final`` runs
    the whole-sequence norm -- the same values."""
    from fastvim_amd import vim_tokens as T
    from fastvim_amd.vim import VisionMamba
    torch.manual_seed(2)
    m = VisionMamba(img_size=64, patch_size=16, depth=1, embed_dim=32, num_classes=4, rms_norm=True, residual_in_fp32=True,
                    fused_add_norm=True, drop_path_rate=0.0, fused_cls=True).cuda()
    g = torch.Generator().manual_seed(4)
    hidden = torch.randn(2, 32, 17, generator=g).cuda().transpose(1, 2)
    residual = torch.randn(2, 17, 32, generator=g).cuda()
    assert not T.add_norm_row_ok(hidden, residual, m.norm_f.weight, None, 8)
    with pytest.raises(RuntimeError, match="add_norm_row_ok"):
        T.add_norm_row(hidden, residual, m.norm_f.weight, None, 1e-5, 8, None, True)
    want = T.add_norm_row(hidden.contiguous(), residual, m.norm_f.weight, None, m.norm_f.eps, 8, None, True)
    assert torch.equal(m._final(hidden, residual), want)
    assert not T.add_norm_row_ok(hidden.contiguous(), residual.bfloat16(), m.norm_f.weight, None, 8)
