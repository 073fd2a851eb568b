"""The MAE token kernels (csrc/mae_tokens.hip, fastvim_amd/mae_tokens.py) against the torch restatement
(tests/mae_tokens_ref.py) and ``MaskedAutoencoderViM`` with ``fused_tokens`` on against off.  Everything is bit-identical
except the gradient of ``mask_token``, a sum whose order differs: it is held to the bound of one fp32 rounding."""
import pytest
import torch

import mae_tokens_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

# fp32 additions a term of d mask_token passes through in the kernels' reduction: none -- mae_decoder_tokens_bwd_kernel adds
# the rows of a workgroup into fp64 partials and mae_decoder_tokens_final_kernel adds the partials in fp64; the only fp32
# rounding is the final conversion of the sum (the "+ 1" of the bound).
C_FP32_ADDS = 0


def mask_token_bound(terms):
    """|err| <= (c + 1) 2^-24 sum|terms|, per channel; ``terms`` (n, D) fp64."""
    return (C_FP32_ADDS + 1) * 2.0 ** -24 * terms.abs().sum(0)


# ------------------------------------------------------------------------------------------------ the plan kernel
PLAN_SHAPES = [(1, 4, 4, 4), (3, 14, 14, 49), (2, 14, 14, 19), (2, 14, 14, 98), (2, 16, 16, 64), (2, 32, 32, 256), (2, 6, 4, 6)]


def _noise(kind, B, L, seed):
    if kind == "tie_free":
        return R.tie_free_noise(B, L, seed)
    if kind == "quantised":
        return R.quantised_noise(B, L, seed)
    return torch.full((B, L), 0.5)


@pytest.mark.parametrize("kind", ["tie_free", "quantised", "all_equal"])
@pytest.mark.parametrize("B,H,W,K", PLAN_SHAPES)
def test_plan_equals_restatement(B, H, W, K, kind):
    from fastvim_amd import mae_tokens
    noise = _noise(kind, B, H * W, seed=H * 1000 + K)
    ref = R.plan_ref(noise, H, W, K)
    assert mae_tokens.mask_plan_ok(noise.cuda(), (H, W), K)
    plan = mae_tokens.mask_plan(noise.cuda(), (H, W), K)
    for k in R.PLAN_KEYS:
        got = getattr(plan, k).cpu()
        assert got.dtype == ref[k].dtype and got.shape == ref[k].shape, (k, got.dtype, got.shape)
        assert torch.equal(got, ref[k]), k
    if kind == "all_equal":
        assert torch.equal(plan.ids_keep.cpu(), torch.arange(K).repeat(B, 1))


def test_plan_of_nan_noise_stays_in_range():
    """Finite noise is the contract; whatever the noise holds, every index is in range and the plan is a permutation."""
    from fastvim_amd import mae_tokens
    B, H, W, K = 2, 14, 14, 49
    noise = R.tie_free_noise(B, H * W, seed=3)
    noise[0, ::3] = float("nan")
    noise[1, :] = float("nan")
    noise[1, 5] = float("-inf")
    noise[0, 1] = -0.0
    plan = mae_tokens.mask_plan(noise.cuda(), (H, W), K)
    L = H * W
    assert torch.equal(plan.ids_restore.cpu().sort(1).values, torch.arange(L).repeat(B, 1))
    assert torch.equal(plan.mask.cpu().sum(1), torch.full((B,), float(L - K)))
    for k, hi in (("ids_keep", L), ("keep_index", L), ("ids_keep_odd", L), ("order", K), ("inverse", K), ("order_index", K),
                  ("inverse_index", K)):
        t = getattr(plan, k).cpu().long()
        assert int(t.min()) >= 0 and int(t.max()) < hi, k
    assert torch.equal(plan.order.cpu().sort(1).values, torch.arange(K).repeat(B, 1))
    assert int(plan.row_index_even.min()) >= 0 and int(plan.row_index_even.max()) < H
    assert int(plan.row_index_odd.min()) >= 0 and int(plan.row_index_odd.max()) < W
    assert int(plan.restore_index.min()) == -1 and int(plan.restore_index.max()) == K - 1


def test_predicate_false_cases_on_the_gpu():
    from fastvim_amd import mae_tokens
    ok = mae_tokens.mask_plan_ok
    n = torch.rand(2, 196, device="cuda")
    assert ok(n, (14, 14), 49)
    assert not ok(n, (14, 14), 2)                                   # K < 3
    assert not ok(n.double(), (14, 14), 49) and not ok(n.bfloat16(), (14, 14), 49)
    assert not ok(torch.rand(2, 392, device="cuda")[:, ::2], (14, 14), 49)      # not contiguous
    assert not ok(torch.rand(1, 33 * 33, device="cuda"), (33, 33), 100)         # L > 1024
    assert not ok(n, (14, 13), 49)                                  # the grid is not the noise's


# ------------------------------------------------------------------------------------------------ fv_tokens_gather
def _rows(B, Lr, D, dtype, seed):
    return torch.randn(B, Lr, D, generator=torch.Generator().manual_seed(seed)).to(dtype).cuda()


def _expand(idx, D):
    return idx.long().unsqueeze(-1).expand(-1, -1, D)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("D", [4, 192, 768, 1280])
def test_gather_equals_torch_gather(D, dtype):
    from fastvim_amd import mae_tokens
    B, Lin, Lout = 3, 37, 11
    x = _rows(B, Lin, D, dtype, seed=D)
    g = torch.Generator().manual_seed(D + 1)
    idx = torch.stack([torch.randperm(Lin, generator=g)[:Lout] for _ in range(B)]).to(torch.int32).cuda()
    out = mae_tokens._gather(x, idx, dtype)
    assert out.dtype == dtype and torch.equal(out, torch.gather(x, 1, _expand(idx, D)))
    # rows with index -1 are exactly zero, the others unchanged
    idx2 = idx.clone()
    idx2[:, ::3] = -1
    out2 = mae_tokens._gather(x, idx2, dtype)
    assert torch.equal(out2[:, ::3], torch.zeros_like(out2[:, ::3]))
    keep = torch.ones(Lout, dtype=torch.bool)
    keep[::3] = False
    assert torch.equal(out2[:, keep], out[:, keep])
    if dtype == torch.float32:                                      # fp32 -> bf16: the one conversion
        assert torch.equal(mae_tokens._gather(x, idx, torch.bfloat16), torch.gather(x, 1, _expand(idx, D)).to(torch.bfloat16))
    else:
        assert torch.equal(mae_tokens._gather(x, idx, torch.float32), torch.gather(x, 1, _expand(idx, D)).float())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("which", ["subset", "permutation"])
def test_gather_gradient_equals_torch_gather_gradient(which, dtype):
    from fastvim_amd import mae_tokens
    B, H, W, K, D = 2, 14, 14, 49, 192
    plan = mae_tokens.mask_plan(R.tie_free_noise(B, H * W, seed=11).cuda(), (H, W), K)
    if which == "subset":
        x, idx, adj, idx64 = _rows(B, H * W, D, dtype, 1), plan.keep_index, plan.restore_index, plan.ids_keep
    else:
        x, idx, adj, idx64 = _rows(B, K, D, dtype, 2), plan.order_index, plan.inverse_index, plan.order
    dout = _rows(B, K, D, dtype, 3)
    a = x.clone().requires_grad_(True)
    out = mae_tokens.gather_tokens(a, idx, adj)
    out.backward(dout)
    b = x.clone().requires_grad_(True)
    ref = torch.gather(b, 1, _expand(idx64, D))
    ref.backward(dout)
    assert torch.equal(out, ref)
    assert a.grad.dtype == b.grad.dtype and torch.equal(a.grad, b.grad)
    if which == "permutation":                                      # each permute is the other's adjoint
        back = mae_tokens.gather_tokens(out.detach(), adj, idx)
        assert torch.equal(back, x)


# ------------------------------------------------------------------------------------------------ decoder tokens
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,L,K,D", [(2, 16, 4, 512), (2, 196, 49, 512)])
def test_decoder_tokens_equal_the_eager_chain(B, L, K, D, dtype):
    from fastvim_amd import mae_tokens
    H = int(L ** 0.5)
    plan = mae_tokens.mask_plan(R.tie_free_noise(B, L, seed=L).cuda(), (H, H), K)
    g = torch.Generator().manual_seed(L + D)
    x = torch.randn(B, K, D, generator=g).to(dtype).cuda()
    mt = (0.02 * torch.randn(1, 1, D, generator=g)).cuda()
    pos = torch.randn(1, L, D, generator=g).cuda()
    dout = torch.randn(B, L, D, generator=g).cuda()
    xa, ma = x.clone().requires_grad_(True), mt.clone().requires_grad_(True)
    assert mae_tokens.decoder_tokens_ok(xa, ma, pos, plan)
    out = mae_tokens.decoder_tokens(xa, ma, pos, plan)
    out.backward(dout)
    xb, mb = x.clone().requires_grad_(True), mt.clone().requires_grad_(True)
    ref = R.decoder_eager(xb, mb, pos, plan.ids_restore)
    ref.backward(dout)
    assert out.dtype == ref.dtype == torch.float32 and torch.equal(out, ref)
    assert xa.grad.dtype == dtype and torch.equal(xa.grad, xb.grad)
    terms = R.decoder_mask_token_terms(dout.cpu(), plan.mask.cpu(), dtype)
    exact, bound = terms.sum(0), mask_token_bound(terms)
    err = (ma.grad.double().cpu().view(-1) - exact).abs()
    err_eager = (mb.grad.double().cpu().view(-1) - exact).abs()
    print(f"d mask_token ({B}, {L}, {K}, {D}) {dtype}: kernel max err / bound {(err / bound).max().item():.3f}, "
          f"eager {(err_eager / bound).max().item():.3f}")
    assert ma.grad.shape == mt.shape and ma.grad.dtype == torch.float32
    assert bool((err <= bound).all()), (err / bound).max().item()
    # deterministic: the same inputs give the same bits
    xc, mc = x.clone().requires_grad_(True), mt.clone().requires_grad_(True)
    mae_tokens.decoder_tokens(xc, mc, pos, plan).backward(dout)
    assert torch.equal(mc.grad, ma.grad)


# ------------------------------------------------------------------------------------------------ the model
def _model(img_size, depth):
    from fastvim_amd.models_mae import mae_FastVim_base_dec512d2b
    torch.manual_seed(21)
    return mae_FastVim_base_dec512d2b(depth=depth, img_size=img_size).cuda().train()


def _step(m, x, noise, fused):
    """One bf16-autocast forward + backward -> (loss, pred, mask, grads, d decoder input)."""
    m.fused_tokens = fused
    for p in m.parameters():
        p.grad = None
    seen = {}

    def pre(_mod, args):
        args[0].register_hook(lambda g: seen.__setitem__("dout", g.detach().clone()))
    h = m.decoder_blocks[0].register_forward_pre_hook(pre)
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss, pred, mask = m(x, mask_ratio=0.75, noise=noise)
        loss.backward()
    finally:
        h.remove()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    return loss.detach(), pred.detach(), mask.detach(), grads, seen["dout"]


@pytest.mark.parametrize("img_size,depth", [(64, 4), (224, 3)])
def test_model_with_fused_tokens_equals_model_without(img_size, depth):
    m = _model(img_size, depth)
    L = (img_size // 16) ** 2
    x = torch.randn(2, 3, img_size, img_size, generator=torch.Generator().manual_seed(5)).cuda()
    noise = R.tie_free_noise(2, L, seed=6).cuda()
    l0, p0, m0, g0, d0 = _step(m, x, noise, False)
    l1, p1, m1, g1, d1 = _step(m, x, noise, True)
    assert torch.equal(l1, l0) and torch.equal(p1, p0) and torch.equal(m1, m0)
    assert p1.dtype == p0.dtype and m1.dtype == m0.dtype == torch.float32
    assert set(g1) == set(g0) and "mask_token" in g0
    for n in g0:
        if n != "mask_token":
            assert torch.equal(g1[n], g0[n]), n
    assert torch.equal(d1, d0) and d0.dtype == torch.float32
    terms = R.decoder_mask_token_terms(d0.cpu(), m0.cpu(), torch.bfloat16)          # decoder_embed's output is bf16 here
    err = (g1["mask_token"].double().cpu().view(-1) - terms.sum(0)).abs()
    bound = mask_token_bound(terms)
    print(f"model {img_size} px: mask_token.grad max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert bool((err <= bound).all())
    # the public pieces keep their types
    m.fused_tokens = True
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        lat, mk, ids_restore = m.forward_encoder(x, 0.75, noise=noise)
    assert ids_restore.dtype == torch.int64 and mk.dtype == torch.float32 and torch.equal(mk, m0)


@pytest.mark.parametrize("case", ["tiny_64_keep4", "tiny_96_keep9"])
def test_golden_mask_with_fused_tokens(case):
    from fastvim_amd.models_mae import MaskedAutoencoderViM
    c = load_golden("mae.pt")[case]
    cfg = c["cfg"]
    m = MaskedAutoencoderViM(img_size=cfg["img_size"], patch_size=cfg["patch_size"], depth=cfg["depth"],
                             embed_dim=cfg["embed_dim"], decoder_embed_dim=cfg["decoder_embed_dim"],
                             decoder_depth=cfg["decoder_depth"], rms_norm=True, residual_in_fp32=True, fused_add_norm=True,
                             fused_tokens=True).cuda()
    m.load_state_dict(c["state_dict"], strict=True)
    x, noise = c["x"].cuda(), c["noise"].cuda()
    assert m._masking(m.patch_embed(x, m.pos_embed), 0.75, noise)[4] is not None        # the plan is taken
    loss, pred, mask = m(x, mask_ratio=0.75, noise=noise)
    assert torch.equal(mask.cpu().float(), c["mask"].float())
    assert abs(loss.item() - c["loss"].item()) <= 2e-5 * max(1.0, abs(c["loss"].item()))


def test_vim_mae_takes_the_plan_in_random_masking():
    """The un-pooled Vim MAE inherits ``random_masking``: same four values with the flag on."""
    from fastvim_amd.fastvim_mae import MaskedAutoencoderViM
    torch.manual_seed(2)
    m = MaskedAutoencoderViM(img_size=64, patch_size=16, depth=1, embed_dim=32, decoder_embed_dim=32, decoder_depth=1,
                             rms_norm=True, residual_in_fp32=True, fused_add_norm=True).cuda()
    x = torch.randn(2, 16, 32, device="cuda")
    noise = R.tie_free_noise(2, 16, seed=9).cuda()
    off = m.random_masking(x, 0.75, noise)
    m.fused_tokens = True
    on = m.random_masking(x, 0.75, noise)
    assert len(on) == 4
    for a, b in zip(on, off):
        assert a.dtype == b.dtype and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ replay
def test_graph_replay_reads_the_plan_from_the_static_noise_buffer():
    """Forward + backward captured with the flag on over a static noise buffer; after another noise is copied in, the
    replay's mask and loss are those of an eager run on that noise: the plan is computed at replay, not frozen at capture."""
    from fastvim_amd.flat import FlatTrainingState
    m = _model(64, 4)
    m.fused_tokens = True
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(8)).cuda()
    n1, n2 = R.tie_free_noise(2, 16, seed=1).cuda(), R.tie_free_noise(2, 16, seed=2).cuda()
    assert not torch.equal(R.plan_ref(n1.cpu(), 4, 4, 4)["mask"], R.plan_ref(n2.cpu(), 4, 4, 4)["mask"])
    flat = FlatTrainingState(m)
    try:
        def fwd_bwd(noise):
            flat.zero_grad()
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss, _, mask = m(x, mask_ratio=0.75, noise=noise)
            loss.backward()
            flat.finish_backward()
            return loss.detach(), mask

        m.fused_tokens = False
        want_loss, want_mask = fwd_bwd(n2)
        want_loss, want_mask, want_grad = want_loss.clone(), want_mask.clone(), flat.grad_flat.clone()
        m.fused_tokens = True
        static = n1.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                fwd_bwd(static)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loss_buf, mask_buf = fwd_bwd(static)
        static.copy_(n2)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(mask_buf, want_mask) and torch.equal(mask_buf.cpu(), R.plan_ref(n2.cpu(), 4, 4, 4)["mask"])
        assert torch.equal(loss_buf, want_loss)
        # gradients: all bits but mask_token's four hundred-odd sums
        diff = (flat.grad_flat != want_grad).sum().item()
        assert diff <= m.mask_token.numel(), diff
    finally:
        flat.close()
