"""The Vim MAE's class-token assembly (csrc/mae_tokens_cls.hip, fastvim_amd/mae_tokens.py: ``encoder_tokens_cls``,
``decoder_tokens_cls``) against the torch restatement (tests/mae_tokens_cls_ref.py, itself held to the model's literal chain
by tests/test_mae_tokens_cls_cpu.py), and ``fastvim_amd.fastvim_mae.MaskedAutoencoderViM`` with ``fused_tokens`` on against
off.  Everything is bit-identical except the gradients of ``cls_token`` and ``mask_token``, sums whose order differs: they
are held to the bound of one fp32 rounding of the fp64 sum of the same terms (``mask_token_bound`` of
tests/test_mae_tokens_gpu.py with no fp32 addition: the kernels accumulate in fp64)."""
import pytest
import torch

import mae_tokens_cls_ref as C
import mae_tokens_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

# (B, H, W, K, D)
CASES = [(3, 4, 4, 3, 32),          # smallest K, c = 1
         (2, 4, 4, 4, 32),          # even K
         (2, 3, 5, 7, 64),          # non-square grid, odd K; 2 x 16 decoder rows: no multiple of the 32-row block
         (2, 4, 4, 16, 32),         # nothing removed: d mask_token is exactly 0
         (1, 32, 32, 256, 512),     # the largest plan; L + 1 = 1025 rows
         (2, 14, 14, 49, 1280)]     # the recipe's grid at the widest model
DTYPES = [torch.bfloat16, torch.float32]


def _plan(B, H, W, K, seed):
    from fastvim_amd import mae_tokens
    return mae_tokens.mask_plan(R.tie_free_noise(B, H * W, seed=seed).cuda(), (H, W), K)


def _assert_sum(got, terms, what):
    """``got`` (D,) fp32 against the fp64 sum of ``terms`` (n, D): one fp32 rounding."""
    exact, bound = terms.sum(0), C.sum_bound(terms)
    err = (got.double().cpu().view(-1) - exact.cpu()).abs()
    print(f"{what}: max err {err.max().item():.3e}, max err / bound {(err / bound.cpu().clamp_min(1e-300)).max().item():.3f}")
    assert bool((err <= bound.cpu()).all()), (what, (err / bound.cpu().clamp_min(1e-300)).max().item())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,H,W,K,D", CASES)
def test_encoder_tokens_cls_equal_the_restatement(B, H, W, K, D, dtype):
    from fastvim_amd import mae_tokens
    L = H * W
    plan = _plan(B, H, W, K, seed=L + K)
    g = torch.Generator().manual_seed(L + D)
    x = torch.randn(B, L, D, generator=g).to(dtype).cuda()
    cls = (0.02 * torch.randn(1, 1, D, generator=g)).cuda()
    pos = torch.randn(1, L + 1, D, generator=g).cuda()
    dout = torch.randn(B, K + 1, D, generator=g).to(dtype).cuda()
    xa, ca = x.clone().requires_grad_(True), cls.clone().requires_grad_(True)
    assert mae_tokens.encoder_tokens_cls_ok(xa, ca, pos, plan)
    out = mae_tokens.encoder_tokens_cls(xa, ca, pos, plan)
    out.backward(dout)
    ref = C.encoder_fwd(x, cls, pos, plan.keep_index)
    assert out.dtype == ref.dtype == dtype and out.shape == (B, K + 1, D) and torch.equal(out, ref)
    dx, terms = C.encoder_bwd(dout, plan.restore_index, K)
    assert xa.grad.dtype == dtype and torch.equal(xa.grad, dx)
    assert ca.grad.shape == cls.shape and ca.grad.dtype == torch.float32
    _assert_sum(ca.grad, terms, f"d cls_token {(B, H, W, K, D)} {dtype}")
    # deterministic: the same inputs give the same bits
    xc, cc = x.clone().requires_grad_(True), cls.clone().requires_grad_(True)
    mae_tokens.encoder_tokens_cls(xc, cc, pos, plan).backward(dout)
    assert torch.equal(cc.grad, ca.grad) and torch.equal(xc.grad, xa.grad)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,H,W,K,D", CASES)
def test_decoder_tokens_cls_equal_the_restatement(B, H, W, K, D, dtype):
    from fastvim_amd import mae_tokens
    L = H * W
    plan = _plan(B, H, W, K, seed=L + K + 1)
    g = torch.Generator().manual_seed(L + D + 1)
    x = torch.randn(B, K + 1, D, generator=g).to(dtype).cuda()
    mt = (0.02 * torch.randn(1, 1, D, generator=g)).cuda()
    pos = torch.randn(1, L + 1, D, generator=g).cuda()
    dout = torch.randn(B, L + 1, D, generator=g).cuda()
    xa, ma = x.clone().requires_grad_(True), mt.clone().requires_grad_(True)
    assert mae_tokens.decoder_tokens_cls_ok(xa, ma, pos, plan)
    out = mae_tokens.decoder_tokens_cls(xa, ma, pos, plan)
    out.backward(dout)
    ref = C.decoder_fwd(x, mt, pos, plan.restore_index)
    assert out.dtype == ref.dtype == torch.float32 and out.shape == (B, L + 1, D) and torch.equal(out, ref)
    dx, terms = C.decoder_bwd(dout, plan.keep_index, plan.restore_index, dtype)
    assert xa.grad.dtype == dtype and torch.equal(xa.grad, dx)
    assert ma.grad.shape == mt.shape and ma.grad.dtype == torch.float32
    assert terms.shape[0] == B * (L - K)
    if K == L:
        assert not ma.grad.any()                                    # nothing removed: exactly zero
    _assert_sum(ma.grad, terms, f"d mask_token {(B, H, W, K, D)} {dtype}")
    xc, mc = x.clone().requires_grad_(True), mt.clone().requires_grad_(True)
    mae_tokens.decoder_tokens_cls(xc, mc, pos, plan).backward(dout)
    assert torch.equal(mc.grad, ma.grad) and torch.equal(xc.grad, xa.grad)


def test_predicates_on_the_gpu():
    from fastvim_amd import mae_tokens
    B, H, W, K, D = 2, 4, 4, 4, 32
    L = H * W
    plan = _plan(B, H, W, K, seed=1)
    x, y = torch.randn(B, L, D, device="cuda"), torch.randn(B, K + 1, D, device="cuda")
    vec, pos = torch.randn(1, 1, D, device="cuda"), torch.randn(1, L + 1, D, device="cuda")
    enc, dec = mae_tokens.encoder_tokens_cls_ok, mae_tokens.decoder_tokens_cls_ok
    assert enc(x, vec, pos, plan) and dec(y, vec, pos, plan)
    for ok, t in ((enc, x), (dec, y)):
        assert not ok(t.cpu(), vec, pos, plan)
        assert not ok(t[..., :30].contiguous(), vec[..., :30].contiguous(), pos[..., :30].contiguous(), plan)
        assert not ok(t, vec, pos[:, 1:].contiguous(), plan)
        assert not ok(t, vec, pos.clone().requires_grad_(True), plan)
        assert not ok(t, vec, pos, _plan(B + 1, H, W, K, seed=1))
    with pytest.raises(RuntimeError, match="encoder_tokens_cls_ok"):
        mae_tokens.encoder_tokens_cls(x, vec, pos[:, 1:].contiguous(), plan)
    with pytest.raises(RuntimeError, match="decoder_tokens_cls_ok"):
        mae_tokens.decoder_tokens_cls(y, vec, pos[:, 1:].contiguous(), plan)


# ------------------------------------------------------------------------------------------------ the model
def _model(img_size=64, embed=32, depth=2):
    from fastvim_amd.fastvim_mae import MaskedAutoencoderViM
    torch.manual_seed(21)
    return MaskedAutoencoderViM(img_size=img_size, patch_size=16, depth=depth, embed_dim=embed, decoder_embed_dim=32,
                                decoder_depth=1, rms_norm=True, residual_in_fp32=True, fused_add_norm=True).cuda().train()


X_DTYPES = {}


def _count_calls(monkeypatch):
    """Counts of the two class-token launches' wrappers, as the model reaches them."""
    from fastvim_amd import mae_tokens
    calls = {"encoder": 0, "decoder": 0}
    enc, dec = mae_tokens.encoder_tokens_cls, mae_tokens.decoder_tokens_cls

    def spy(key, fn):
        def call(x, *rest):
            calls[key] += 1
            X_DTYPES[key] = x.dtype                                 # the type of the tokens the launch was given
            return fn(x, *rest)
        return call
    monkeypatch.setattr(mae_tokens, "encoder_tokens_cls", spy("encoder", enc))
    monkeypatch.setattr(mae_tokens, "decoder_tokens_cls", spy("decoder", dec))
    return calls


def _step(m, x, noise, fused, amp):
    """One forward + backward -> (loss, pred, mask, ids_restore, grads, d encoder tokens, d decoder input)."""
    m.fused_tokens = fused
    for p in m.parameters():
        p.grad = None
    seen = {}

    def pre(key):
        return lambda _mod, args: args[0].register_hook(lambda g: seen.__setitem__(key, g.detach().clone())) and None
    hooks = [m.layers[0].register_forward_pre_hook(pre("enc")), m.decoder_blocks[0].register_forward_pre_hook(pre("dec"))]
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            latent, mask, ids_restore, plan = m._encode(x, 0.75, noise=noise)
            pred = m.forward_decoder(latent, ids_restore, plan=plan)
            loss = m._loss(x, pred, mask)
            loss2, pred2, mask2 = m(x, mask_ratio=0.75, noise=noise)
        assert (plan is not None) is fused
        assert torch.equal(loss2, loss) and torch.equal(pred2, pred) and torch.equal(mask2, mask)       # forward() is that sequence
        loss.backward()
    finally:
        for h in hooks:
            h.remove()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    return loss.detach(), pred.detach(), mask.detach(), ids_restore.detach(), grads, seen["enc"], seen["dec"]


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("img_size,embed", [(64, 32), (96, 64)])
def test_model_with_fused_tokens_equals_model_without(img_size, embed, amp, monkeypatch):
    m = _model(img_size, embed)
    calls = _count_calls(monkeypatch)
    L = (img_size // 16) ** 2
    K = int(L * 0.25)
    x = torch.randn(2, 3, img_size, img_size, generator=torch.Generator().manual_seed(5)).cuda()
    noise = R.tie_free_noise(2, L, seed=6).cuda()
    l0, p0, m0, r0, g0, e0, d0 = _step(m, x, noise, False, amp)
    assert calls == {"encoder": 0, "decoder": 0}
    l1, p1, m1, r1, g1, e1, d1 = _step(m, x, noise, True, amp)
    assert calls == {"encoder": 2, "decoder": 2}                   # (_step runs the forward twice)
    assert torch.equal(l1, l0) and torch.equal(p1, p0) and torch.equal(m1, m0) and torch.equal(r1, r0)
    assert p1.dtype == p0.dtype and m1.dtype == m0.dtype == torch.float32 and r1.dtype == r0.dtype == torch.int64
    assert p1.shape == (2, L, 16 * 16 * 3)
    assert set(g1) == set(g0) and {"mask_token", "cls_token"} <= set(g0)
    for n in g0:
        if n not in ("mask_token", "cls_token"):
            assert torch.equal(g1[n], g0[n]), n
    # the types of the patch embedding's and of decoder_embed's output, as the launches saw them: autograd rounds the rows of
    # d mask_token to the latter before it adds them
    edt, ddt = X_DTYPES["encoder"], X_DTYPES["decoder"]
    assert edt in (torch.float32, torch.bfloat16) and ddt in (torch.float32, torch.bfloat16)
    if not amp:
        assert edt == ddt == torch.float32
    assert e1.dtype == e0.dtype == edt and torch.equal(e1, e0) and e0.shape == (2, K + 1, embed)
    assert d0.dtype == torch.float32 and torch.equal(d1, d0) and d0.shape == (2, L + 1, 32)
    _assert_sum(g1["cls_token"], e0[:, K // 2].double(), f"model {img_size} px cls_token.grad")
    _assert_sum(g1["mask_token"], d0[:, :L][m0.bool()].to(ddt).double(), f"model {img_size} px mask_token.grad")


@pytest.mark.parametrize("case", ["mae_vim_64_keep4", "mae_vim_96_keep9"])
def test_mae_vim_fp32_vs_reference_golden_with_fused_tokens(case, monkeypatch):
    """tests/test_baselines_gpu.py::test_mae_vim_fp32_vs_reference_golden with the flag on: the same assertions and
    tolerances, and the plan is taken -- both class-token launches run."""
    from fastvim_amd.fastvim_mae import MaskedAutoencoderViM

    def _err(a, b):
        return (a.double().cpu() - b.double().cpu()).abs().max().item()
    c = load_golden("baselines.pt")[case]
    cfg = c["cfg"]
    m = MaskedAutoencoderViM(img_size=cfg["img_size"], patch_size=cfg["patch_size"], depth=cfg["depth"],
                             embed_dim=cfg["embed_dim"], decoder_embed_dim=cfg["decoder_embed_dim"],
                             decoder_depth=cfg["decoder_depth"], rms_norm=True, residual_in_fp32=True,
                             fused_add_norm=True, fused_tokens=True).cuda()
    m.load_state_dict(c["state_dict"], strict=True)
    calls = _count_calls(monkeypatch)
    x, noise = c["x"].cuda(), c["noise"].cuda()
    assert m._mask_with_cls(m.patch_embed(x, m.pos_embed[:, 1:, :]), 0.75, noise)[3] is not None        # the plan is taken
    assert calls == {"encoder": 1, "decoder": 0}
    loss, pred, mask = m(x, mask_ratio=0.75, noise=noise)
    assert calls == {"encoder": 2, "decoder": 1}
    assert torch.equal(mask.cpu().float(), c["mask"].float())
    assert abs(loss.item() - c["loss"].item()) <= 2e-5 * max(1.0, abs(c["loss"].item()))
    assert _err(pred, c["pred"]) <= 2e-5 * max(1.0, c["pred"].abs().max().item()), _err(pred, c["pred"])
    loss.backward()
    params = dict(m.named_parameters())
    for k, gref in c["grads"].items():
        e = _err(params[k].grad, gref)
        assert e <= 2e-4 * max(1e-3, gref.abs().max().item()), (k, e, gref.abs().max().item())
    with torch.autocast("cuda", dtype=torch.bfloat16):
        lb, pb, _ = m(x, mask_ratio=0.75, noise=noise)
    assert calls == {"encoder": 3, "decoder": 2}
    assert abs(lb.item() - c["loss"].item()) <= 5e-2 * max(1.0, abs(c["loss"].item()))


# ------------------------------------------------------------------------------------------------ replay
def test_graph_replay_reads_the_plan_from_the_static_noise_buffer():
    """Forward + backward captured with the flag on over a static noise buffer; after another noise is copied in, the
    replay's mask and loss are those of an eager run on that noise: the plan is computed at replay, not frozen at capture."""
    from fastvim_amd.flat import FlatTrainingState
    m = _model(64, 32)
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
        # gradients: all bits but the sums of mask_token and cls_token
        diff = (flat.grad_flat != want_grad).sum().item()
        assert diff <= m.mask_token.numel() + m.cls_token.numel(), diff
    finally:
        flat.close()
