"""``VimMAEPretrainStep`` (fastvim_amd/mae_step.py) -- the graph-replayed MAE pre-training step of the Vim baseline,
``fastvim_amd.fastvim_mae.MaskedAutoencoderViM`` -- against a hand-written eager loop with the same mechanics; the mirror of
tests/test_mae_step_gpu.py for the model with a class token."""
import json
import os
import subprocess
import sys

import pytest
import torch

import mask_noise_ref as N

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, SIZE, DEPTH, EMBED = 3, 64, 4, 32
N_MICRO = 6
LR = 1e-3
CASES = [(1, 1, False), (2, 3, True), (3, 2, True)]          # (accum_iter, n_segments, use_graph)


def _model(seed=21):
    from fastvim_amd.fastvim_mae import MaskedAutoencoderViM
    torch.manual_seed(seed)
    return MaskedAutoencoderViM(img_size=SIZE, patch_size=16, depth=DEPTH, embed_dim=EMBED, decoder_embed_dim=32,
                                decoder_depth=1, rms_norm=True, residual_in_fp32=True, fused_add_norm=True).cuda().train()


def _images(kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "u8":
        return torch.randint(0, 256, (B, 3, SIZE, SIZE), generator=g, dtype=torch.uint8).cuda()
    return torch.randn(B, 3, SIZE, SIZE, generator=g).cuda()


def _make(kind="float", seed=21):
    from fastvim_amd import pixels
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    m = _model(seed)
    if kind == "u8":
        pixels.attach_pixel_norm(m, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    flat = FlatTrainingState(m)
    opt = FlatAdamW(flat, m, lr=LR, betas=(0.9, 0.95), ema_decay=0.999)
    return m, flat, opt


def _loop(kind, accum, n_micro, seed):
    """The plain loop.  -> (losses, masks, (model, flat, opt, sampler))."""
    from fastvim_amd.mae_tokens import MaskSampler
    m, flat, opt = _make(kind)
    s = MaskSampler(seed=seed)
    losses, masks = [], []
    for it in range(n_micro):
        x = _images(kind, 100 + it)
        s.sample()
        if it % accum == 0:
            flat.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss, _, mask = m(x, mask_ratio=0.75, sampler=s)
        loss.backward()
        flat.finish_backward()
        if it % accum == accum - 1:
            opt.step(grad_scale=1.0 / accum)
        losses.append(loss.item())
        masks.append(mask.cpu().clone())
    return losses, masks, (m, flat, opt, s)


def _run_step(kind, accum, n_seg, graph, n_micro, seed):
    from fastvim_amd.mae_step import VimMAEPretrainStep
    from fastvim_amd.mae_tokens import MaskSampler
    m, flat, opt = _make(kind)
    s = MaskSampler(seed=seed)
    x = _images(kind, 0)                                        # what the warm-up steps of the capture run on
    step = VimMAEPretrainStep(m, flat, opt, x, s, mask_ratio=0.75, accum_iter=accum, n_segments=n_seg, use_graph=graph)
    assert step.use_graph is graph and step.K == n_seg and step.accum_iter == accum
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
                losses, masks, (m, flat, opt, s) = _loop(kind, accum, N_MICRO, seed=11)
                cache[(kind, accum)] = (losses, masks, flat.param_flat.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(),
                                        opt.ema.clone(), opt.step_t.item(), s.last())
                flat.close()
            finally:
                gemm_mod.FILL = saved
        return cache[(kind, accum)]
    return get


def _assert_equals_loop(kind, accum, n_seg, graph, loops, monkeypatch):
    import fastvim_amd.gemm as gemm_mod
    ref_losses, ref_masks, ref_params, ref_m1, ref_m2, ref_ema, ref_t, ref_last = loops(kind, accum)
    monkeypatch.setattr(gemm_mod, "FILL", False)
    losses, masks, ran, (m, flat, opt, s, step) = _run_step(kind, accum, n_seg, graph, N_MICRO, seed=11)
    try:
        assert losses == ref_losses, (losses, ref_losses)
        assert all(torch.equal(a, b) for a, b in zip(masks, ref_masks))
        assert len({tuple(mk.flatten().tolist()) for mk in masks}) == N_MICRO          # six different masks
        assert torch.equal(flat.param_flat, ref_params) and torch.equal(opt.ema, ref_ema)
        assert torch.equal(opt.exp_avg, ref_m1) and torch.equal(opt.exp_avg_sq, ref_m2)
        assert opt.step_t.item() == ref_t == float(N_MICRO // accum) and s.last() == ref_last == (11, N_MICRO)
        assert ran == [i % accum == accum - 1 for i in range(N_MICRO)]
    finally:
        flat.close()


@pytest.mark.parametrize("accum,n_seg,graph", CASES)
def test_step_equals_loop_bit_for_bit(accum, n_seg, graph, loops, monkeypatch):
    _assert_equals_loop("float", accum, n_seg, graph, loops, monkeypatch)


def test_step_on_uint8_batches_equals_loop_bit_for_bit(loops, monkeypatch):
    """``attach_pixel_norm`` serves the model's patch embedding (fastvim_amd/vim.py: ``PatchEmbed``): the uint8 batch goes
    through the step as it goes through the loop."""
    _assert_equals_loop("u8", 2, 2, True, loops, monkeypatch)


def test_replays_draw_new_masks():
    from fastvim_amd.mae_step import VimMAEPretrainStep
    from fastvim_amd.mae_tokens import MaskSampler
    m, flat, opt = _make()
    s = MaskSampler(seed=6)
    step = VimMAEPretrainStep(m, flat, opt, _images("float", 3), s, accum_iter=4, n_segments=1)
    try:
        assert step.use_graph
        masks = []
        for _ in range(2):
            s.sample()
            step.micro_step()
            masks.append(step.mask.cpu().clone())
        assert not torch.equal(masks[0], masks[1])
        for c, got in zip((1, 2), masks):
            assert torch.equal(got, N.plan(6, c, B, 4, 4, 4)["mask"]), c
    finally:
        flat.close()


def test_construction_leaves_no_trace():
    from fastvim_amd.mae_step import VimMAEPretrainStep
    from fastvim_amd.mae_tokens import MaskSampler
    m, flat, opt = _make()
    s = MaskSampler(seed=6)
    s.sample()
    torch.manual_seed(99)
    before = [t.clone() for t in (flat.param_flat, flat.shadow_flat, opt.exp_avg, opt.exp_avg_sq, opt.ema, opt.step_t)]
    cpu_rng, gpu_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
    try:
        step = VimMAEPretrainStep(m, flat, opt, _images("float", 3), s, accum_iter=2, n_segments=2)
        assert step.use_graph
        torch.cuda.synchronize()
        after = (flat.param_flat, flat.shadow_flat, opt.exp_avg, opt.exp_avg_sq, opt.ema, opt.step_t)
        assert all(torch.equal(a, b) for a, b in zip(after, before))
        assert torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(), gpu_rng)
        assert s.last() == (6, 1) and s.block().tolist() == [6, 0, 1, 0]
    finally:
        flat.close()


def test_construction_checks():
    from fastvim_amd.mae_step import MAEPretrainStep, VimMAEPretrainStep
    from fastvim_amd.mae_tokens import MaskSampler
    from fastvim_amd.models_mae import mae_FastVim_base_dec512d2b
    s, x = MaskSampler(seed=0), _images("float", 3)
    torch.manual_seed(1)
    fastvim = mae_FastVim_base_dec512d2b(depth=1, img_size=SIZE).cuda().train()
    with pytest.raises(TypeError, match="VimMAEPretrainStep.*_embed_masked_cls"):
        VimMAEPretrainStep(fastvim, None, None, x, s)
    vim = _model()
    with pytest.raises(TypeError, match="MAEPretrainStep: fastvim_amd.fastvim_mae.MaskedAutoencoderViM has no _embed_masked\\(\\)"):
        MAEPretrainStep(vim, None, None, x, s)
    m, flat, opt = _make()
    try:
        with pytest.raises(ValueError, match="accum_iter"):
            VimMAEPretrainStep(m, flat, opt, x, s, accum_iter=0)
        with pytest.raises(ValueError, match="masking plan"):
            VimMAEPretrainStep(m, flat, opt, x, s, mask_ratio=0.9)          # one token kept
        m.eval()
        with pytest.raises(ValueError, match="eval"):
            VimMAEPretrainStep(m, flat, opt, x, s)
    finally:
        flat.close()


def test_exchange_behind_the_last_micro_batch_only_and_the_tokens_in_its_last_bucket():
    from fastvim_amd.mae_step import VimMAEPretrainStep
    from fastvim_amd.mae_tokens import MaskSampler
    m, flat, opt = _make()
    s = MaskSampler(seed=1)
    x = _images("float", 3)
    step = VimMAEPretrainStep(m, flat, opt, x, s, accum_iter=3, n_segments=2)
    calls = []
    launch, finish = step.exchange.launch, step.exchange.finish
    step.exchange.launch = lambda k: (calls.append(("launch", k)), launch(k))[1]
    step.exchange.finish = lambda mean=True: (calls.append(("finish", mean)), finish(mean=mean))[1]
    try:
        # the flat layout of this model: cls_token and mask_token both lie in the unit in front of the block stack, which is
        # part of the bucket launched LAST -- behind the backward graph that completes cls_token.grad
        lo, hi = flat.buckets(2)[-1]["bounds"]
        first_block = min(o for n, o in flat.offsets.items() if n.startswith("layers."))
        for name in ("cls_token", "mask_token"):
            assert lo == 0 and flat.offsets[name] < first_block <= hi, (name, flat.offsets[name], first_block, lo, hi)
        assert step.runs[-1][0] == 0                                # ... which is the run that starts at block 0
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


def test_resume_inside_a_group_continues_bit_for_bit(monkeypatch):
    """Three micro-batches of groups of two, the state taken (mid-group), loaded into a fresh set, three more: the same
    losses, masks and weights as six in a row."""
    import fastvim_amd.gemm as gemm_mod
    from fastvim_amd.mae_step import VimMAEPretrainStep
    from fastvim_amd.mae_tokens import MaskSampler
    monkeypatch.setattr(gemm_mod, "FILL", False)
    want_losses, want_masks, _, (m0, f0, o0, s0, _) = _run_step("float", 2, 2, True, 6, seed=13)
    first_losses, first_masks, _, (m1, f1, o1, s1, st1) = _run_step("float", 2, 2, True, 3, seed=13)
    state = {"step": st1.state_dict(), "sampler": s1.state_dict(), "opt": o1.state_dict(), "params": f1.param_flat.clone()}
    assert state["step"]["micro"] == 1 and state["step"]["grad_flat"] is not None
    m2, f2, o2 = _make(seed=77)                                  # another initialisation: everything must come from the state
    s2 = MaskSampler(seed=0)
    x = _images("float", 0)
    st2 = VimMAEPretrainStep(m2, f2, o2, x, s2, accum_iter=2, n_segments=2)
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
import fastvim_amd.gemm as gemm_mod
from fastvim_amd.fastvim_mae import MaskedAutoencoderViM
from fastvim_amd.flat import FlatAdamW, FlatTrainingState
from fastvim_amd.mae_step import VimMAEPretrainStep
from fastvim_amd.mae_tokens import MaskSampler
gemm_mod.FILL = False                                   # the parent compares bits with an unsegmented eager run
torch.cuda.set_device(0)
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:" + port, rank=rank, world_size=2)
torch.manual_seed(21)                                   # the same initialisation on both ranks
m = MaskedAutoencoderViM(img_size=64, patch_size=16, depth=4, embed_dim=32, decoder_embed_dim=32, decoder_depth=1,
                         rms_norm=True, residual_in_fp32=True, fused_add_norm=True).cuda().train()
flat = FlatTrainingState(m)
opt = FlatAdamW(flat, m, lr=1e-3, betas=(0.9, 0.95), ema_decay=0.999)
s = MaskSampler(seed=rank)
x = torch.zeros(3, 3, 64, 64, device="cuda")
step = VimMAEPretrainStep(m, flat, opt, x, s, accum_iter=1, n_segments=3, warmup=1)
launches, summed = [], []
launch, finish = step.exchange.launch, step.exchange.finish
step.exchange.launch = lambda k: (launches.append(k), launch(k))[1]
def finish_and_keep(mean=True):
    r = finish(mean=mean)
    summed.append(flat.grad_flat.detach().clone())       # what the optimizer graph reads
    return r
step.exchange.finish = finish_and_keep
x.copy_(torch.randn(3, 3, 64, 64, generator=torch.Generator().manual_seed(1000 + rank)))
s.sample()
loss = step.micro_step()
torch.cuda.synchronize()
dist.barrier()
torch.save({"grad": summed[0].cpu(), "params": flat.param_flat.cpu()}, out)
print(json.dumps({"rank": rank, "graph": step.use_graph, "world": step.exchange.world_size, "gscale": step._gscale,
                  "launches": launches, "n_finish": len(summed), "loss": loss.item(), "step_t": opt.step_t.item(),
                  "mask": step.mask.cpu().tolist()}))
flat.close()
dist.destroy_process_group()
'''


def _local_gradient(rank, monkeypatch):
    """What rank ``rank`` of the script adds to the exchange: the flat gradient of its first micro-batch, from a plain
    eager forward + backward of the same model, images and masks."""
    import fastvim_amd.gemm as gemm_mod
    from fastvim_amd.mae_tokens import MaskSampler
    monkeypatch.setattr(gemm_mod, "FILL", False)
    m, flat, opt = _make()
    try:
        s = MaskSampler(seed=rank)
        x = torch.randn(B, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(1000 + rank)).cuda()
        s.sample()
        flat.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss, _, mask = m(x, mask_ratio=0.75, sampler=s)
        loss.backward()
        flat.finish_backward()
        torch.cuda.synchronize()
        return flat.grad_flat.detach().cpu().clone(), loss.item(), dict(flat.offsets)
    finally:
        flat.close()


def test_two_ranks_on_one_gpu(tmp_path, monkeypatch):
    """Two ranks share GPU 0 over gloo, a fresh child each, seeds = rank, three buckets: the gradient the optimizer graph
    reads after ``finish()`` is, bit for bit, the sum of the two ranks' own gradients -- ``cls_token``'s, complete only after
    the last backward graph, and ``mask_token``'s included: a bucket launched too early would miss what came later."""
    script = tmp_path / "vim_mae_step_rank.py"
    script.write_text(_RANK_SCRIPT)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, str(r), "29563", str(tmp_path / f"rank{r}.pt")], env=env,
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
        assert o["graph"] is True and o["world"] == 2 and o["gscale"] == 0.5 and o["step_t"] == 1.0
        assert o["launches"] == [0, 1, 2] and o["n_finish"] == 1
    assert a["mask"] != b["mask"]
    (g0, l0, offsets), (g1, l1, _) = _local_gradient(0, monkeypatch), _local_gradient(1, monkeypatch)
    assert (a["loss"], b["loss"]) == (l0, l1)
    ra, rb = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    want = g0 + g1                                                   # two fp32 terms: one rounding, whatever the order
    for name in ("cls_token", "mask_token"):
        o, n = offsets[name], EMBED
        assert g0[o:o + n].abs().sum() > 0 and g1[o:o + n].abs().sum() > 0, name
        assert torch.equal(ra["grad"][o:o + n], want[o:o + n]), name
    assert torch.equal(ra["grad"], want) and torch.equal(rb["grad"], want)
    assert torch.isfinite(ra["params"]).all() and torch.equal(ra["params"], rb["params"])
