"""The keyed masking noise and plan (csrc/mask_noise.h, csrc/mae_tokens.hip) against the numpy restatement
(tests/mask_noise_ref.py), ``MaskedAutoencoderViM`` with ``sampler=``, and ``MAEPretrainStep`` (fastvim_amd/mae_step.py)
against a hand-written eager loop with the same mechanics."""
import json
import os
import subprocess
import sys

import pytest
import torch

import mae_tokens_ref as R
import mask_noise_ref as N

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COUNTERS = (1, 2 ** 32 + 5)
SEEDS = (0, 2 ** 40 + 3)


def _sampler(seed, counter):
    from fastvim_amd.mae_tokens import MaskSampler
    s = MaskSampler(seed=seed)
    s.set_counter(counter)
    return s


# ------------------------------------------------------------------------------------------------ noise
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("counter", COUNTERS)
@pytest.mark.parametrize("B,L", [(3, 15), (2, 16), (2, 196), (1, 1024)])
def test_noise_equals_restatement(B, L, counter, seed):
    got = _sampler(seed, counter).noise(B, L)
    assert got.dtype == torch.float32 and got.shape == (B, L)
    assert torch.equal(got.cpu(), N.noise(seed, counter, B, L))


def test_sample_advances_the_block():
    from fastvim_amd.mae_tokens import MaskSampler
    s = MaskSampler(seed=3)
    first = s.noise(2, 16)                       # counter 0
    s.sample()
    assert torch.equal(s.noise(2, 16).cpu(), N.noise(3, 1, 2, 16)) and torch.equal(first.cpu(), N.noise(3, 0, 2, 16))
    assert s.block().dtype == torch.int32 and s.block().tolist() == [3, 0, 1, 0]


# ------------------------------------------------------------------------------------------------ keyed plan
def _plan_cases():
    out = []
    for H, W in ((3, 5), (4, 4), (14, 14), (32, 32), (16, 16)):
        L = H * W
        for K in sorted({3, int(L / 4), L - 1}):
            if K >= 3:
                out.append((2 if L > 16 else 3, H, W, K))
    return out


def _check_plan(sampler, seed, counter, B, H, W, K):
    from fastvim_amd import mae_tokens
    plan = mae_tokens.mask_plan_keyed(sampler, B, (H, W), K)
    via_noise = mae_tokens.mask_plan(sampler.noise(B, H * W), (H, W), K)
    ref = N.plan(seed, counter, B, H, W, K)
    assert plan.token_size == (H, W)
    for k in R.PLAN_KEYS:
        got = getattr(plan, k)
        assert got.dtype == ref[k].dtype and got.shape == ref[k].shape, (k, got.dtype, got.shape)
        assert torch.equal(got, getattr(via_noise, k)), k
        assert torch.equal(got.cpu(), ref[k]), k


@pytest.mark.parametrize("seed,counter", [(0, 1), (2 ** 40 + 3, 2 ** 32 + 5)])
@pytest.mark.parametrize("B,H,W,K", _plan_cases())
def test_keyed_plan_equals_plan_of_the_noise(B, H, W, K, seed, counter):
    _check_plan(_sampler(seed, counter), seed, counter, B, H, W, K)


@pytest.mark.parametrize("K", [3, 256, 1023])
def test_keyed_plan_ranks_equal_values_by_token_index(K):
    c = N.TIE_CASE
    row = N.noise(c["seed"], c["counter"], c["B"], c["L"])[c["sample"]]
    assert row.unique().numel() < row.numel()
    _check_plan(_sampler(c["seed"], c["counter"]), c["seed"], c["counter"], c["B"], 32, 32, K)


def test_keyed_plan_refuses_what_the_predicate_refuses():
    from fastvim_amd import mae_tokens
    s = _sampler(0, 1)
    for args in ((2, (4, 4), 2), (2, (33, 32), 100), (0, (4, 4), 4)):
        assert not mae_tokens.plan_shape_ok(*args)
        with pytest.raises(RuntimeError, match="plan_shape_ok"):
            mae_tokens.mask_plan_keyed(s, *args)


# ------------------------------------------------------------------------------------------------ the eager model
def _model(img_size=64, depth=4, seed=21):
    from fastvim_amd.models_mae import mae_FastVim_base_dec512d2b
    torch.manual_seed(seed)
    return mae_FastVim_base_dec512d2b(depth=depth, img_size=img_size).cuda().train()


def _images(kind, seed, B=2, size=64):
    g = torch.Generator().manual_seed(seed)
    if kind == "u8":
        return torch.randint(0, 256, (B, 3, size, size), generator=g, dtype=torch.uint8).cuda()
    return torch.randn(B, 3, size, size, generator=g).cuda()


def _attach(m):
    from fastvim_amd import pixels
    pixels.attach_pixel_norm(m, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def _fwd_bwd(m, x, **kw):
    for p in m.parameters():
        p.grad = None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss, pred, mask = m(x, mask_ratio=0.75, **kw)
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    return loss.detach().clone(), pred.detach().clone(), mask.detach().clone(), grads


@pytest.mark.parametrize("kind", ["float", "u8"])
def test_model_with_sampler_equals_model_with_its_noise(kind):
    m = _model()
    if kind == "u8":
        _attach(m)
    x = _images(kind, 5)
    s = _sampler(4, 9)
    assert m.fused_tokens is False                              # the sampler is the opt-in
    l1, p1, m1, g1 = _fwd_bwd(m, x, sampler=s)
    m.fused_tokens = True
    l0, p0, m0, g0 = _fwd_bwd(m, x, noise=s.noise(2, 16))
    assert torch.equal(l1, l0) and torch.equal(p1, p0) and torch.equal(m1, m0)
    assert set(g1) == set(g0) and "mask_token" in g1
    for n in g0:
        assert torch.equal(g1[n], g0[n]), n
    assert torch.equal(m1.cpu(), N.plan(4, 9, 2, 4, 4, 4)["mask"])
    with pytest.raises(ValueError, match="sampler"):
        m(x, noise=s.noise(2, 16), sampler=s)


def test_predicate_false_paths_give_the_same_mask():
    """Tokens the plan kernels do not take -- a width that is no multiple of 4, fewer than 3 kept -- go through the torch
    composition on ``sampler.noise``: the mask of the restatement either way."""
    m = _model()
    s = _sampler(4, 9)
    narrow = torch.randn(2, 16, 6, device="cuda")               # D % 4 != 0
    xm, mask, ids_restore, ids_keep = m.random_masking(narrow, 0.75, sampler=s)
    ref = N.plan(4, 9, 2, 4, 4, 4)
    assert torch.equal(mask.cpu(), ref["mask"]) and torch.equal(ids_keep.cpu(), ref["ids_keep"])
    assert torch.equal(xm, torch.gather(narrow, 1, ids_keep.unsqueeze(-1).expand(-1, -1, 6)))
    assert m._masking(narrow, 0.75, sampler=s)[4] is None
    wide = torch.randn(2, 16, 8, device="cuda")
    assert m._masking(wide, 0.75, sampler=s)[4] is not None
    _, mask2, _, keep2 = m.random_masking(wide, 0.9, sampler=s)                  # one token kept: below the conv halo
    shuffle = torch.argsort(N.noise(4, 9, 2, 16), dim=1, stable=True)
    assert torch.equal(keep2.cpu(), shuffle[:, :1]) and mask2.sum().item() == 2 * 15


# ------------------------------------------------------------------------------------------------ the step
ACCUM_CASES = [(1, 1, True, "float"), (1, 2, True, "float"), (2, 2, True, "float"), (2, 2, False, "float"), (2, 2, True, "u8")]
N_OPT_STEPS = 3
LR = 1e-3


def _make(kind="float", seed=21):
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    m = _model(seed=seed)
    if kind == "u8":
        _attach(m)
    flat = FlatTrainingState(m)
    opt = FlatAdamW(flat, m, lr=LR, betas=(0.9, 0.95), ema_decay=0.999)
    return m, flat, opt


def _loop(kind, accum, n_micro, seed, loss_scale=1.0, grad_scale=None, start=0, state=None):
    """The hand-written eager loop.  -> (losses, masks, (model, flat, opt, sampler))."""
    from fastvim_amd.mae_tokens import MaskSampler
    m, flat, opt = _make(kind)
    s = MaskSampler(seed=seed)
    gs = 1.0 / accum if grad_scale is None else grad_scale
    losses, masks = [], []
    for it in range(n_micro):
        x = _images(kind, 100 + it)
        s.sample()
        if it % accum == 0:
            flat.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss, _, mask = m(x, mask_ratio=0.75, sampler=s)
        (loss * loss_scale if loss_scale != 1.0 else loss).backward()
        flat.finish_backward()
        if it % accum == accum - 1:
            opt.step(grad_scale=gs)
        losses.append(loss.item())
        masks.append(mask.cpu().clone())
    return losses, masks, (m, flat, opt, s)


def _run_step(kind, accum, n_seg, graph, n_micro, seed):
    from fastvim_amd.mae_step import MAEPretrainStep
    from fastvim_amd.mae_tokens import MaskSampler
    m, flat, opt = _make(kind)
    s = MaskSampler(seed=seed)
    x = _images(kind, 0)                                        # what the warm-up steps of the capture run on
    step = MAEPretrainStep(m, flat, opt, x, s, mask_ratio=0.75, accum_iter=accum, n_segments=n_seg, use_graph=graph)
    assert step.use_graph is graph and step.K == n_seg
    losses, masks, ran = [], [], []
    for it in range(n_micro):
        x.copy_(_images(kind, 100 + it))
        s.sample()
        losses.append(step.micro_step().item())
        masks.append(step.mask.cpu().clone())
        ran.append(step.optimizer_ran)
    torch.cuda.synchronize()
    return losses, masks, ran, (m, flat, opt, s, step)


@pytest.fixture(scope="module")
def loops():
    """The reference loops with ``gemm.FILL`` off, once per (kind, accum_iter); read-only."""
    import fastvim_amd.gemm as gemm_mod
    cache = {}

    def get(kind, accum):
        if (kind, accum) not in cache:
            saved, gemm_mod.FILL = gemm_mod.FILL, False
            try:
                losses, masks, (m, flat, opt, s) = _loop(kind, accum, N_OPT_STEPS * accum, seed=11)
                cache[(kind, accum)] = (losses, masks, flat.param_flat.clone(), opt.ema.clone(), opt.step_t.item(), s.last())
                flat.close()
            finally:
                gemm_mod.FILL = saved
        return cache[(kind, accum)]
    return get


@pytest.mark.parametrize("accum,n_seg,graph,kind", ACCUM_CASES)
def test_step_equals_loop_bit_for_bit(accum, n_seg, graph, kind, loops, monkeypatch):
    import fastvim_amd.gemm as gemm_mod
    ref_losses, ref_masks, ref_params, ref_ema, ref_t, ref_last = loops(kind, accum)
    monkeypatch.setattr(gemm_mod, "FILL", False)
    losses, masks, ran, (m, flat, opt, s, step) = _run_step(kind, accum, n_seg, graph, N_OPT_STEPS * accum, seed=11)
    try:
        assert losses == ref_losses, (losses, ref_losses)
        assert all(torch.equal(a, b) for a, b in zip(masks, ref_masks))
        assert torch.equal(flat.param_flat, ref_params) and torch.equal(opt.ema, ref_ema)
        assert opt.step_t.item() == ref_t == float(N_OPT_STEPS) and s.last() == ref_last == (11, N_OPT_STEPS * accum)
        assert ran == [i % accum == accum - 1 for i in range(N_OPT_STEPS * accum)]
    finally:
        flat.close()


def _assert_close_trajectories(losses, ref_losses, p, p_ref, n_steps):
    """The bounds of the inexact branch of tests/test_pipeline_gpu.py (5 steps of lr 1e-3 there: 2e-3 on the losses, 5.5e-3 max
    and 2e-5 mean on the weights), scaled by steps x lr: AdamW turns a rounding-level difference of a near-zero gradient into
    a step of up to lr."""
    scale = n_steps * LR / (5 * 1e-3)
    d = (p - p_ref).abs()
    print(f"max |loss diff| {max(abs(a - b) for a, b in zip(losses, ref_losses)):.3e} (bound {2e-3 * scale:.1e}), weights max "
          f"{d.max().item():.3e} (bound {5.5e-3 * scale:.1e}) mean {d.mean().item():.3e} (bound {2e-5 * scale:.1e})")
    torch.testing.assert_close(torch.tensor(losses), torch.tensor(ref_losses), rtol=0, atol=2e-3 * scale)
    assert d.max().item() <= 5.5e-3 * scale
    assert d.mean().item() <= 2e-5 * scale


def test_step_with_the_shipped_fill_default_agrees_to_rounding():
    losses_ref, _, (m0, f0, o0, _) = _loop("float", 2, N_OPT_STEPS * 2, seed=11)
    losses, _, _, (m, flat, opt, s, step) = _run_step("float", 2, 2, True, N_OPT_STEPS * 2, seed=11)
    try:
        _assert_close_trajectories(losses, losses_ref, flat.param_flat, f0.param_flat, N_OPT_STEPS)
    finally:
        flat.close(); f0.close()


def test_step_agrees_with_lightnings_mechanics():
    """Lightning backpropagates ``loss / accum_iter`` per micro-batch and steps on the sum; the step seeds every backward
    with 1 and scales inside the optimizer kernel.  Scaling by a power of two commutes with rounding except for flushed
    denormals, so this is held to the rounding bounds, not to equality."""
    losses_ref, _, (m0, f0, o0, _) = _loop("float", 2, N_OPT_STEPS * 2, seed=11, loss_scale=0.5, grad_scale=1.0)
    losses, _, _, (m, flat, opt, s, step) = _run_step("float", 2, 2, True, N_OPT_STEPS * 2, seed=11)
    try:
        _assert_close_trajectories(losses, losses_ref, flat.param_flat, f0.param_flat, N_OPT_STEPS)
    finally:
        flat.close(); f0.close()


def test_no_exchange_before_the_last_micro_batch():
    from fastvim_amd.mae_step import MAEPretrainStep
    from fastvim_amd.mae_tokens import MaskSampler
    m, flat, opt = _make()
    s = MaskSampler(seed=1)
    x = _images("float", 3)
    step = MAEPretrainStep(m, flat, opt, x, s, accum_iter=3, n_segments=2)
    calls = []
    launch, finish = step.exchange.launch, step.exchange.finish
    step.exchange.launch = lambda k: (calls.append(("launch", k)), launch(k))[1]
    step.exchange.finish = lambda mean=True: (calls.append(("finish", mean)), finish(mean=mean))[1]
    try:
        for group in range(2):
            for i in range(3):
                s.sample()
                step.micro_step()
                assert step.optimizer_ran is (i == 2)
                if i < 2:
                    assert calls == [], (group, i, calls)
            assert calls == [("launch", 0), ("launch", 1), ("finish", False)], calls
            calls.clear()
        torch.cuda.synchronize()
        assert opt.step_t.item() == 2.0
    finally:
        flat.close()


def test_replays_draw_new_masks():
    from fastvim_amd.mae_step import MAEPretrainStep
    from fastvim_amd.mae_tokens import MaskSampler
    m, flat, opt = _make()
    s = MaskSampler(seed=6)
    step = MAEPretrainStep(m, flat, opt, _images("float", 3), s, accum_iter=4, n_segments=1)
    try:
        assert step.use_graph
        masks = []
        for _ in range(2):
            s.sample()
            step.micro_step()
            masks.append(step.mask.cpu().clone())
        assert not torch.equal(masks[0], masks[1])
        for c, got in zip((1, 2), masks):
            assert torch.equal(got, N.plan(6, c, 2, 4, 4, 4)["mask"]), c
    finally:
        flat.close()


def test_construction_leaves_no_trace():
    from fastvim_amd.mae_step import MAEPretrainStep
    from fastvim_amd.mae_tokens import MaskSampler
    m, flat, opt = _make()
    s = MaskSampler(seed=6)
    s.sample()
    torch.manual_seed(99)
    before = [t.clone() for t in (flat.param_flat, flat.shadow_flat, opt.exp_avg, opt.exp_avg_sq, opt.ema, opt.step_t)]
    cpu_rng, gpu_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
    try:
        step = MAEPretrainStep(m, flat, opt, _images("float", 3), s, accum_iter=2, n_segments=2)
        assert step.use_graph
        torch.cuda.synchronize()
        after = (flat.param_flat, flat.shadow_flat, opt.exp_avg, opt.exp_avg_sq, opt.ema, opt.step_t)
        assert all(torch.equal(a, b) for a, b in zip(after, before))
        assert torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(), gpu_rng)
        assert s.last() == (6, 1) and s.block().tolist() == [6, 0, 1, 0]
    finally:
        flat.close()


def test_construction_checks():
    from fastvim_amd.fastvim_mae import MaskedAutoencoderViM as VimMAE
    from fastvim_amd.mae_step import MAEPretrainStep
    from fastvim_amd.mae_tokens import MaskSampler
    m, flat, opt = _make()
    s, x = MaskSampler(seed=0), _images("float", 3)
    try:
        with pytest.raises(ValueError, match="accum_iter"):
            MAEPretrainStep(m, flat, opt, x, s, accum_iter=0)
        with pytest.raises(ValueError, match="masking plan"):
            MAEPretrainStep(m, flat, opt, x, s, mask_ratio=0.9)             # one token kept
        m.eval()
        with pytest.raises(ValueError, match="eval"):
            MAEPretrainStep(m, flat, opt, x, s)
    finally:
        flat.close()
    vim = VimMAE(img_size=64, patch_size=16, depth=1, embed_dim=32, decoder_embed_dim=32, decoder_depth=1, rms_norm=True,
                 residual_in_fp32=True, fused_add_norm=True).cuda().train()
    with pytest.raises(TypeError, match="_embed_masked"):
        MAEPretrainStep(vim, None, None, x, s)


def test_resume_inside_a_group_continues_bit_for_bit(monkeypatch):
    """Three micro-batches of groups of two, the state taken (mid-group), loaded into a fresh set, three more: the same
    losses, masks and weights as six in a row."""
    import fastvim_amd.gemm as gemm_mod
    from fastvim_amd.mae_step import MAEPretrainStep
    from fastvim_amd.mae_tokens import MaskSampler
    monkeypatch.setattr(gemm_mod, "FILL", False)
    want_losses, want_masks, _, (m0, f0, o0, s0, _) = _run_step("float", 2, 2, True, 6, seed=13)
    first_losses, first_masks, _, (m1, f1, o1, s1, st1) = _run_step("float", 2, 2, True, 3, seed=13)
    state = {"step": st1.state_dict(), "sampler": s1.state_dict(), "opt": o1.state_dict(), "params": f1.param_flat.clone()}
    assert state["step"]["micro"] == 1 and state["step"]["grad_flat"] is not None
    m2, f2, o2 = _make(seed=77)                                  # another initialisation: everything must come from the state
    s2 = MaskSampler(seed=0)
    x = _images("float", 0)
    st2 =MAEPretrainStep(m2, f2, o2, x, s2, accum_iter=2, n_segments=2)
    try:
        with torch.no_grad():
            f2.param_flat.copy_(state["params"])
        f2.refresh_shadow()
        o2.load_state_dict(state["opt"])
        s2.load_state_dict(state["sampler"])
        st2.load_state_dict(state["step"])
        losses, masks = list(first_losses), list(first_masks)
        for it in range(3, 6):
            x.copy_(_images("float", 100 + it))
            s2.sample()
            losses.append(st2.micro_step().item())
            masks.append(st2.mask.cpu().clone())
        torch.cuda.synchronize()
        assert losses == want_losses and all(torch.equal(a, b) for a, b in zip(masks, want_masks))
        assert torch.equal(f2.param_flat, f0.param_flat) and torch.equal(o2.ema, o0.ema)
        assert o2.step_t.item() == o0.step_t.item() == 3.0 and s2.last() == s0.last()
    finally:
        f0.close(); f1.close(); f2.close()


# ------------------------------------------------------------------------------------------------ two ranks on one GPU
_RANK_SCRIPT = r'''
import os, sys, json
sys.path.insert(0, sys.argv[1])
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
rank, port, out = int(sys.argv[2]), sys.argv[3], sys.argv[4]
import torch, torch.distributed as dist
from fastvim_amd.flat import FlatAdamW, FlatTrainingState
from fastvim_amd.mae_step import MAEPretrainStep
from fastvim_amd.mae_tokens import MaskSampler
from fastvim_amd.models_mae import mae_FastVim_base_dec512d2b
torch.cuda.set_device(0)
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:" + port, rank=rank, world_size=2)
torch.manual_seed(21)                                   # the same initialisation on both ranks
m = mae_FastVim_base_dec512d2b(depth=4, img_size=64).cuda().train()
flat = FlatTrainingState(m)
opt = FlatAdamW(flat, m, lr=1e-3, betas=(0.9, 0.95), ema_decay=0.999)
s = MaskSampler(seed=rank)
x = torch.zeros(2, 3, 64, 64, device="cuda")
step = MAEPretrainStep(m, flat, opt, x, s, accum_iter=2, n_segments=2, warmup=1)
launches, masks, losses = [], [], []
launch = step.exchange.launch
step.exchange.launch = lambda k: (launches.append(len(losses)), launch(k))[1]
for it in range(4):
    x.copy_(torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(1000 * rank + it)))
    s.sample()
    loss = step.micro_step()
    masks.append(step.mask.cpu().tolist())
    losses.append(loss.item())
torch.cuda.synchronize()
dist.barrier()
torch.save(flat.param_flat.cpu(), out)
print(json.dumps({"rank": rank, "graph": step.use_graph, "world": step.exchange.world_size, "gscale": step._gscale,
                  "launches": launches, "masks": masks, "losses": losses, "step_t": opt.step_t.item()}))
flat.close()
dist.destroy_process_group()
'''


def test_two_ranks_on_one_gpu(tmp_path):
    """Two ranks share GPU 0 over gloo, a fresh child each: ``accum_iter=2``, two groups, seeds = rank.  The buckets are
    exchanged in the last micro-batch of a group only; the ranks drew different masks and end with identical weights."""
    script = tmp_path / "mae_step_rank.py"
    script.write_text(_RANK_SCRIPT)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, str(r), "29561", str(tmp_path / f"params{r}.pt")], env=env,
                              cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    outs = []
    try:
        for p in procs:
            so, se = p.communicate(timeout=240)
            assert p.returncode == 0, se[-3000:]
            outs.append(json.loads([l for l in so.splitlines() if l.startswith("{")][-1]))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    a, b = sorted(outs, key=lambda o: o["rank"])
    for o in (a, b):
        assert o["graph"] is True and o["world"] == 2 and o["gscale"] == 0.25 and o["step_t"] == 2.0
        assert o["launches"] == [1, 1, 3, 3]                        # both buckets, behind micro-batches 1 and 3 only
        assert all(v == v for v in o["losses"])
    assert a["masks"] != b["masks"]
    pa, pb = torch.load(tmp_path / "params0.pt"), torch.load(tmp_path / "params1.pt")
    assert torch.isfinite(pa).all() and torch.equal(pa, pb)
