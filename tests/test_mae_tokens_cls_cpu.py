"""The restatement of the Vim MAE's class-token assembly (tests/mae_tokens_cls_ref.py) against the literal chains of
fastvim_amd/fastvim_mae.py, on the CPU, bit for bit -- forward, and ``dx`` through autograd -- and the pure-Python predicates
of ``encoder_tokens_cls`` / ``decoder_tokens_cls``.  No GPU and no library needed."""
import pytest
import torch

import mae_tokens_cls_ref as C
import mae_tokens_ref as R

GRIDS = [(4, 4), (3, 5), (6, 6)]
DTYPES = [torch.float32, torch.bfloat16]


def _cases():
    out = []
    for H, W in GRIDS:
        for K in sorted({3, 4, 7, 9, H * W}):
            out.append((H, W, K))
    return out


def _inputs(H, W, K, D, Dd, dtype, seed):
    B, L = 2, H * W
    g = torch.Generator().manual_seed(seed)
    plan = R.plan_ref(R.tie_free_noise(B, L, seed=seed + 1), H, W, K)
    x = torch.randn(B, L, D, generator=g).to(dtype)
    cls = 0.02 * torch.randn(1, 1, D, generator=g)
    pos = torch.randn(1, L + 1, D, generator=g)
    y = torch.randn(B, K + 1, Dd, generator=g).to(dtype)
    mt = 0.02 * torch.randn(1, 1, Dd, generator=g)
    dpos = torch.randn(1, L + 1, Dd, generator=g)
    return plan, x, cls, pos, y, mt, dpos, g


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,W,K", _cases())
def test_encoder_restatement_equals_the_chain(H, W, K, dtype):
    plan, x, cls, pos, *_, g = _inputs(H, W, K, 8, 12, dtype, seed=H * 100 + K)
    xa = x.clone().requires_grad_(True)
    ref = C.encoder_chain(xa, cls, pos, plan["ids_keep"])
    out = C.encoder_fwd(x, cls, pos, plan["keep_index"])
    assert out.dtype == ref.dtype == dtype and out.shape == (2, K + 1, 8) and torch.equal(out, ref)
    dout = torch.randn(2, K + 1, 8, generator=g).to(dtype)
    ref.backward(dout)
    dx, cls_terms = C.encoder_bwd(dout, plan["restore_index"], K)
    assert dx.dtype == xa.grad.dtype and torch.equal(dx, xa.grad)
    assert torch.equal(cls_terms, dout[:, K // 2].double())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,W,K", _cases())
def test_decoder_restatement_equals_the_chain(H, W, K, dtype):
    plan, _, _, _, y, mt, dpos, g = _inputs(H, W, K, 8, 12, dtype, seed=H * 100 + K + 50)
    L = H * W
    ya, ma = y.clone().requires_grad_(True), mt.clone().requires_grad_(True)
    ref = C.decoder_chain(ya, ma, dpos, plan["ids_restore"])
    out = C.decoder_fwd(y, mt, dpos, plan["restore_index"])
    assert out.dtype == ref.dtype == torch.float32 and out.shape == (2, L + 1, 12) and torch.equal(out, ref)
    dout = torch.randn(2, L + 1, 12, generator=g)
    ref.backward(dout)
    dx, terms = C.decoder_bwd(dout, plan["keep_index"], plan["restore_index"], dtype)
    assert dx.dtype == ya.grad.dtype == dtype and torch.equal(dx, ya.grad)
    # the terms are the ones autograd sums: 2 (L - K) rows, and their fp64 sum is what d mask_token approximates
    assert terms.shape == (2 * (L - K), 12)
    if K == L:
        assert ma.grad is None or not ma.grad.any()
    else:
        err = (ma.grad.double().view(-1) - terms.sum(0)).abs()
        # eager adds in fp32 in some order: at most (n - 1) fp32 additions of partial sums bounded by sum|terms|
        assert bool((err <= terms.shape[0] * 2.0 ** -24 * terms.abs().sum(0)).all())


# ------------------------------------------------------------------------------------------------ predicates
class _OnGpu(torch.Tensor):
    """A CPU tensor that answers ``is_cuda`` with True: the predicates are pure Python, so everything behind their first
    question can be asked without a GPU."""
    is_cuda = property(lambda self: True)


def _gpu(t):
    return torch.Tensor._make_subclass(_OnGpu, t)


def _plan(B, H, W, K):
    from fastvim_amd.mae_tokens import TokenPlan
    p = R.plan_ref(R.tie_free_noise(B, H * W, seed=3), H, W, K)
    return TokenPlan(token_size=(H, W), **{k: p[k] for k in R.PLAN_KEYS})


@pytest.mark.parametrize("which", ["encoder", "decoder"])
def test_predicates(which):
    from fastvim_amd import mae_tokens
    B, H, W, K, D = 2, 4, 4, 4, 8
    L = H * W
    plan = _plan(B, H, W, K)
    ok = mae_tokens.encoder_tokens_cls_ok if which == "encoder" else mae_tokens.decoder_tokens_cls_ok
    rows = L if which == "encoder" else K + 1
    x = torch.randn(B, rows, D)
    vec, pos = torch.randn(1, 1, D), torch.randn(1, L + 1, D)
    assert ok(_gpu(x), vec, pos, plan)                                   # the case every refusal below departs from
    assert ok(_gpu(x.bfloat16()), vec, pos, plan)
    assert not ok(x, vec, pos, plan)                                     # a CPU tensor
    assert not ok(_gpu(torch.randn(B, rows, 6)), torch.randn(1, 1, 6), torch.randn(1, L + 1, 6), plan)      # D % 4 != 0
    assert not ok(_gpu(x), vec, torch.randn(1, L, D), plan)              # L rows of pos_embed: no class slot
    assert not ok(_gpu(x), vec, pos.clone().requires_grad_(True), plan)  # pos_embed must not require grad
    assert not ok(_gpu(x), vec, pos, _plan(B + 1, H, W, K))              # a plan of another batch size
    assert not ok(_gpu(x.double()), vec, pos, plan) and not ok(_gpu(x.half()), vec, pos, plan)
    assert not ok(_gpu(x), vec.double(), pos, plan) and not ok(_gpu(x), torch.randn(1, 1, D + 4), pos, plan)
    if which == "decoder":                                               # (the encoder's x does not depend on K)
        assert not ok(_gpu(x), vec, pos, _plan(B, H, W, K + 1))          # a plan of another K
    assert not ok(_gpu(x), vec, pos, _plan(B, 3, 5, K))                  # a plan of another grid
    assert not ok(_gpu(torch.randn(B, rows + 1, D)), vec, pos, plan)     # rows that are not the plan's
    assert not ok(_gpu(x[0]), vec, pos, plan)
    fn = mae_tokens.encoder_tokens_cls if which == "encoder" else mae_tokens.decoder_tokens_cls
    with pytest.raises(RuntimeError, match=f"{which}_tokens_cls_ok"):
        fn(x, vec, pos, plan)


def test_vim_mae_on_the_cpu_keeps_the_torch_chain():
    """``fused_tokens`` on a CPU model: every predicate says no, the chain runs, the values are those of the flag off."""
    from fastvim_amd.fastvim_mae import MaskedAutoencoderViM
    torch.manual_seed(2)
    m = MaskedAutoencoderViM(img_size=64, patch_size=16, depth=0, embed_dim=32, decoder_embed_dim=32, decoder_depth=0,
                             rms_norm=True, residual_in_fp32=True, fused_add_norm=True)
    x = torch.randn(2, 16, 32)
    noise = R.tie_free_noise(2, 16, seed=9)
    off = m._mask_with_cls(x, 0.75, noise)
    m.fused_tokens = True
    on = m._mask_with_cls(x, 0.75, noise)
    assert off[3] is None and on[3] is None
    for a, b in zip(on[:3], off[:3]):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert torch.equal(on[0], C.encoder_chain(x, m.cls_token, m.pos_embed, R.plan_ref(noise, 4, 4, 4)["ids_keep"]))
    for name in ("_embed_masked_cls", "_run_layers_cls", "_tail_cls"):
        assert callable(getattr(m, name))
    assert m._embed_masked is None and m._run_layers is None and m._tail is None
