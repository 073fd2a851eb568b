"""The ChannelVim baseline (``fastvim_amd.models_channel_mamba.VisionMamba``) through ``SegmentedTrainStep`` with a channel
sampler: ``fused_cls`` on against off, the replayed step with ``hcs=`` against a hand-written eager loop whose model draws
inside ``forward`` (float batches; a uint8 buffer), replays that read the index array, what constructing the step leaves
behind, the flat layout behind the last backward graph, two ranks on one GPU, and ``ValidationStep``."""
import json
import os
import random
import subprocess
import sys

import pytest
import torch

import norm_checks as NC
from mae_tokens_cls_ref import sum_bound

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, SIZE, CHANNELS, DEPTH, EMBED, CLASSES = 4, 32, 3, 4, 32, 10
P = (SIZE // 16) ** 2
N_STEPS = 6
LR = 1e-3
MEAN3, STD3 = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CASES = [(1, False), (3, True), (2, True)]                    # (n_segments, use_graph)
# ``random.seed(0)`` and six ``hcs.draw(3)``: every count, and subsets that are no prefix of the channels -- a family captured
# with range(c) must read the device array to get these right
DRAWS = [[0, 1], [1, 2], [1, 2], [0, 2], [0, 1, 2], [2]]


def test_the_draws_are_the_ones_this_file_counts_on():
    from fastvim_amd import hcs
    random.seed(0)
    draws = [hcs.draw(CHANNELS) for _ in range(N_STEPS)]
    assert draws == DRAWS
    assert {len(d) for d in draws} == {1, 2, 3} and any(d != list(range(len(d))) for d in draws)


def _model(fused_cls, seed=21):
    from fastvim_amd.models_channel_mamba import VisionMamba
    torch.manual_seed(seed)
    return VisionMamba(img_size=SIZE, patch_size=16, channels=CHANNELS, depth=DEPTH, embed_dim=EMBED, num_classes=CLASSES,
                       rms_norm=True, residual_in_fp32=True, fused_add_norm=True, if_cls_token=True, if_abs_pos_embed=True,
                       drop_path_rate=0.1, fused_cls=fused_cls).cuda().train()


def _make(fused_cls=True, u8=False, seed=21):
    from fastvim_amd import pixels
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    m = _model(fused_cls, seed)
    if u8:
        pixels.attach_pixel_norm(m, MEAN3, STD3, formula="albumentations")
    flat = FlatTrainingState(m)
    nd = {n for n, p in m.named_parameters() if p.ndim <= 1 or n.endswith(".bias") or n in m.no_weight_decay()}
    return m, flat, FlatAdamW(flat, m, lr=LR, weight_decay=0.05, no_decay=nd, ema_decay=0.999)


def _images(u8, seed):
    g = torch.Generator().manual_seed(seed)
    if u8:
        return torch.randint(0, 256, (B, CHANNELS, SIZE, SIZE), generator=g, dtype=torch.uint8).cuda()
    return torch.randn(B, CHANNELS, SIZE, SIZE, generator=g).cuda()


def _soft_targets(seed):
    return torch.softmax(torch.randn(B, CLASSES, generator=torch.Generator().manual_seed(seed)), -1).cuda()


def _labels(seed):
    return torch.randint(0, CLASSES, (B,), generator=torch.Generator().manual_seed(seed)).cuda()


# ------------------------------------------------------------------------------------------------ fused_cls on / off
def test_fused_cls_on_equals_off(monkeypatch):
    import fastvim_amd.gemm as gemm_mod
    from fastvim_amd.hcs import ChannelSampler
    monkeypatch.setattr(gemm_mod, "FILL", False)
    on, off = _model(True), _model(False)
    assert on.fused_cls is True and off.fused_cls is False
    assert all(torch.equal(a, b) for a, b in zip(on.parameters(), off.parameters()))
    x, tgt = _images(False, 1), _soft_targets(2)
    sampler = ChannelSampler(CHANNELS)
    sampler.set([0, 2])
    M = P * 2
    p = M // 2
    kept = {}

    def run(m):
        torch.manual_seed(7)                                   # the same DropPath draws
        with torch.autocast("cuda", dtype=torch.bfloat16):
            tokens, _ = m._embed(x, hcs=sampler)
            tokens.retain_grad()
            scale = m.drop_path.__dict__["_pre"].clone()       # what _final's row_scale() will take
            h, res = m._run_layers(tokens, None, 0, DEPTH)
            feat = m._final(h, res)
            feat.retain_grad()
            logits = m._head(feat)
        loss = -(tgt * torch.log_softmax(logits.float(), -1)).sum(-1).mean()
        loss.backward()
        kept[m] = (tokens, h.detach(), res.detach(), scale, feat)
        return logits.detach()

    la, lb = run(on), run(off)
    assert torch.equal(la, lb)
    tokens, h, res, scale, feat = kept[on]
    assert tokens.shape == (B, M + 1, EMBED) and torch.equal(tokens, kept[off][0]) and torch.equal(feat, kept[off][4])
    assert torch.equal(tokens[:, p], on.cls_token.detach().to(tokens.dtype).expand(B, 1, EMBED)[:, 0])
    assert torch.equal(tokens.grad, kept[off][0].grad)
    summed = ("cls_token", "norm_f.weight")
    goff = dict(off.named_parameters())
    for name, prm in on.named_parameters():
        assert prm.grad is not None and goff[name].grad is not None, name
        if name not in summed:
            assert torch.equal(prm.grad, goff[name].grad), name
    # the two sums: one fp32 rounding of the fp64 sum of the same terms / the dw bound on the B class rows
    cls_terms = tokens.grad[:, p].double()
    err = (on.cls_token.grad.double().view(-1) - cls_terms.sum(0)).abs()
    assert bool((err <= sum_bound(cls_terms)).all())
    assert on.cls_token.grad.abs().sum() > 0
    ref = NC.reference(h[:, p], on.norm_f.weight, None, res[:, p], scale, on.norm_f.eps, True, feat.grad, None)
    msg = NC.check_dw(on.norm_f.weight.grad, ref)
    assert not msg, msg
    assert not NC.check_dw(off.norm_f.weight.grad, ref)
    # the undrawn channel's embedding row got no gradient on either side
    assert not on.patch_embed.channel_embed.weight.grad[1].any()


# ------------------------------------------------------------------------------------------------ step against loop
def _loop(u8):
    """The plain loop, eager: the model called as the recipe calls it, drawing its channels inside ``forward`` from Python's
    ``random`` -> (losses, params, m1, m2, ema, step count, the next value of the random stream)."""
    from fastvim_amd.losses import SoftTargetCrossEntropy
    m, flat, opt = _make(u8=u8)
    x = _images(u8, 0)
    crit = SoftTargetCrossEntropy()
    random.seed(0)
    torch.manual_seed(7)
    losses = []
    for it in range(N_STEPS):
        x.copy_(_images(u8, 100 + it))
        tgt = _soft_targets(200 + it)
        flat.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits = m(x)
        loss = crit(logits, tgt)
        loss.backward()
        flat.finish_backward()
        opt.step()
        losses.append(loss.item())
    out = (losses, flat.param_flat.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.ema.clone(), opt.step_t.item(),
           random.random())
    flat.close()
    return out


@pytest.fixture(scope="module")
def loops():
    """The reference loops with ``gemm.FILL`` off, once per kind; read-only."""
    import fastvim_amd.gemm as gemm_mod
    cache = {}

    def get(u8):
        if u8 not in cache:
            saved, gemm_mod.FILL = gemm_mod.FILL, False
            try:
                cache[u8] = _loop(u8)
            finally:
                gemm_mod.FILL = saved
        return cache[u8]
    return get


def _run_step(u8, n_seg, graph):
    from fastvim_amd.hcs import ChannelSampler
    from fastvim_amd.losses import SoftTargetCrossEntropy
    from fastvim_amd.pipeline import SegmentedTrainStep
    m, flat, opt = _make(u8=u8)
    x, tgt = _images(u8, 0), _soft_targets(0)
    sampler = ChannelSampler(CHANNELS)
    random.seed(0)
    torch.manual_seed(7)
    step = SegmentedTrainStep(m, flat, opt, SoftTargetCrossEntropy(), x, tgt, n_segments=n_seg, use_graph=graph, warmup=2,
                              hcs=sampler)
    assert step.use_graph is graph and step.K == n_seg
    if graph:
        assert sorted(step.families) == [1, 2, 3] and len({id(f[0]) for f in step.families.values()}) == 3
    losses, draws = [], []
    for it in range(N_STEPS):
        x.copy_(_images(u8, 100 + it))
        tgt.copy_(_soft_targets(200 + it))
        draws.append(sampler.sample())
        losses.append(step.step().item())
    torch.cuda.synchronize()
    assert draws == DRAWS, draws
    return losses, m, flat, opt, random.random()


def _assert_equals_loop(u8, n_seg, graph, loops, monkeypatch):
    import fastvim_amd.gemm as gemm_mod
    ref_losses, ref_params, ref_m1, ref_m2, ref_ema, ref_t, ref_next = loops(u8)
    monkeypatch.setattr(gemm_mod, "FILL", False)
    losses, m, flat, opt, nxt = _run_step(u8, n_seg, graph)
    try:
        assert nxt == ref_next                                 # the loop's model drew the same six subsets
        assert losses == ref_losses, (losses, ref_losses)
        assert all(v == v for v in losses) and len(set(losses)) == N_STEPS
        assert torch.equal(flat.param_flat, ref_params) and torch.equal(opt.ema, ref_ema)
        assert torch.equal(opt.exp_avg, ref_m1) and torch.equal(opt.exp_avg_sq, ref_m2)
        assert opt.step_t.item() == ref_t == float(N_STEPS)
    finally:
        flat.close()


@pytest.mark.parametrize("n_seg,graph", CASES)
def test_step_with_sampler_equals_loop_bit_for_bit(n_seg, graph, loops, monkeypatch):
    _assert_equals_loop(False, n_seg, graph, loops, monkeypatch)


def test_step_from_uint8_with_sampler_equals_loop_bit_for_bit(loops, monkeypatch):
    """A uint8 buffer after ``attach_pixel_norm(..., formula="albumentations")``: the table row of the SOURCE channel inside
    the per-channel unfold, whatever subset the array holds."""
    _assert_equals_loop(True, 3, True, loops, monkeypatch)


def test_replays_read_the_index_array_on_the_same_batch():
    """The same images and targets, lr 0 and the RNG put back: only the subset differs -- two subsets of EQUAL count, so the
    same family of graphs replays both times."""
    from fastvim_amd.hcs import ChannelSampler
    from fastvim_amd.losses import SoftTargetCrossEntropy
    from fastvim_amd.pipeline import SegmentedTrainStep
    m, flat, opt = _make()
    x, tgt = _images(False, 4), _soft_targets(5)
    sampler = ChannelSampler(CHANNELS)
    try:
        step = SegmentedTrainStep(m, flat, opt, SoftTargetCrossEntropy(), x, tgt, n_segments=2, use_graph=True, warmup=1,
                                  hcs=sampler)
        assert step.use_graph
        opt.set_lr(0.0)
        state = torch.cuda.get_rng_state()
        losses = []
        for subset in ([0, 1], [1, 2], [1, 2], [2, 0]):
            sampler.set(subset)
            assert step.families[2][0] is step.families[sampler.count][0]
            torch.cuda.set_rng_state(state)
            losses.append(step.step().item())
        assert losses[0] != losses[1] and losses[1] == losses[2] and losses[3] not in losses[:3], losses
    finally:
        flat.close()


# ------------------------------------------------------------------------------------------------ construction
def test_construction_leaves_no_trace():
    from fastvim_amd.hcs import ChannelSampler
    from fastvim_amd.losses import SoftTargetCrossEntropy
    from fastvim_amd.pipeline import SegmentedTrainStep
    m, flat, opt = _make()
    x, tgt = _images(False, 3), _soft_targets(4)
    sampler = ChannelSampler(CHANNELS)
    sampler.set([2, 0])
    torch.manual_seed(99)
    random.seed(5)
    before = [t.clone() for t in (flat.param_flat, flat.shadow_flat, opt.exp_avg, opt.exp_avg_sq, opt.ema, opt.step_t)]
    cpu_rng, gpu_rng, py_rng = torch.get_rng_state(), torch.cuda.get_rng_state(), random.getstate()
    try:
        step = SegmentedTrainStep(m, flat, opt, SoftTargetCrossEntropy(), x, tgt, n_segments=2, use_graph=True, warmup=2,
                                  hcs=sampler)
        assert step.use_graph
        torch.cuda.synchronize()
        after = (flat.param_flat, flat.shadow_flat, opt.exp_avg, opt.exp_avg_sq, opt.ema, opt.step_t)
        assert all(torch.equal(a, b) for a, b in zip(after, before))
        assert torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(), gpu_rng)
        assert random.getstate() == py_rng
        assert sampler.last() == [2, 0] and sampler.block().tolist()[:2] == [2, 0]
    finally:
        flat.close()


def test_cls_token_and_patch_embedding_lie_in_the_last_bucket():
    """The layout ``flat.make_exchange(3)`` cuts: the bucket launched behind the LAST backward graph -- the one that
    completes the gradients of everything in front of the block stack -- holds ``cls_token``, ``pos_embed`` and the patch
    embedding whole.  A host-side assertion."""
    m, flat, opt = _make()
    try:
        ex = flat.make_exchange(3)
        assert len(ex.layers) == 3 and ex.layers[-1][0] == 0
        lo, hi = flat.buckets(3)[-1]["bounds"]
        first_block = min(o for n, o in flat.offsets.items() if n.startswith("layers."))
        sizes = {n: p.numel() for n, p in m.named_parameters()}
        for name in ("cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias",
                     "patch_embed.channel_embed.weight"):
            o = flat.offsets[name]
            assert lo == 0 and lo <= o and o + sizes[name] <= first_block <= hi, (name, o, sizes[name], first_block, lo, hi)
    finally:
        flat.close()


# ------------------------------------------------------------------------------------------------ validation
def test_validation_step_with_fused_cls_equals_without():
    """Evaluation embeds every channel and never draws from the sampler's stream."""
    from fastvim_amd.evaluate import ValidationStep
    results, logits = [], []
    x, y = _images(False, 30), _labels(31)
    for fused in (True, False):
        m, flat, opt = _make(fused_cls=fused)
        try:
            val = ValidationStep(m, flat, opt, x.clone(), y.clone(), ema=True, warmup=1)
            val.reset()
            val.step(n_valid=B)
            val.step(n_valid=B - 1)
            torch.cuda.synchronize()
            results.append(val.compute())
            m.eval()
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                logits.append(m(x))
                tokens, _ = m._embed(x)
                assert tokens.shape == (B, P * CHANNELS + 1, EMBED)
            m.train()
        finally:
            flat.close()
    a, b = results
    assert a["n"] == b["n"] == 2 * B - 1
    for key in ("val_acc", "val_loss", "val_acc_macro", "val_acc_ema", "val_loss_ema"):
        assert a[key] == b[key] and a[key] == a[key], key
    assert torch.equal(logits[0], logits[1])


# ------------------------------------------------------------------------------------------------ two ranks on one GPU
_RANK_SCRIPT = r'''
import os, sys, json
sys.path.insert(0, sys.argv[1])
rank, port, out = int(sys.argv[2]), sys.argv[3], sys.argv[4]
import fastvim_amd                                      # (first: it prepares the process for graph capture)
import torch, torch.distributed as dist
import fastvim_amd.gemm as gemm_mod
from fastvim_amd.flat import FlatAdamW, FlatTrainingState
from fastvim_amd.hcs import ChannelSampler
from fastvim_amd.losses import SoftTargetCrossEntropy
from fastvim_amd.models_channel_mamba import VisionMamba
from fastvim_amd.pipeline import SegmentedTrainStep
gemm_mod.FILL = False                                   # the parent compares bits with an unsegmented eager run
torch.cuda.set_device(0)
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:" + port, rank=rank, world_size=2)
torch.manual_seed(21)                                   # the same initialisation on both ranks
m = VisionMamba(img_size=32, patch_size=16, channels=3, depth=4, embed_dim=32, num_classes=10, rms_norm=True,
                residual_in_fp32=True, fused_add_norm=True, if_cls_token=True, if_abs_pos_embed=True, drop_path_rate=0.1,
                fused_cls=True).cuda().train()
flat = FlatTrainingState(m)
nd = {n for n, p in m.named_parameters() if p.ndim <= 1 or n.endswith(".bias") or n in m.no_weight_decay()}
opt = FlatAdamW(flat, m, lr=1e-3, weight_decay=0.05, no_decay=nd, ema_decay=0.999)
x = torch.zeros(4, 3, 32, 32, device="cuda")
tgt = torch.full((4, 10), 0.1, device="cuda")
sampler = ChannelSampler(3)
torch.manual_seed(50 + rank)                            # the DropPath stream of this rank
step = SegmentedTrainStep(m, flat, opt, SoftTargetCrossEntropy(), x, tgt, n_segments=3, use_graph=True, warmup=1, hcs=sampler)
launches, summed = [], []
launch, finish = step.exchange.launch, step.exchange.finish
step.exchange.launch = lambda k: (launches.append(k), launch(k))[1]
def finish_and_keep(mean=True):
    r = finish(mean=mean)
    summed.append(flat.grad_flat.detach().clone())       # what the optimizer graph reads
    return r
step.exchange.finish = finish_and_keep
x.copy_(torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(1000 + rank)))
tgt.copy_(torch.softmax(torch.randn(4, 10, generator=torch.Generator().manual_seed(2000 + rank)), -1))
sampler.set([[0, 2], [1]][rank])                        # each rank its own subset, of its own count
loss = step.step()
torch.cuda.synchronize()
dist.barrier()
torch.save({"grad": summed[0].cpu(), "params": flat.param_flat.cpu()}, out)
print(json.dumps({"rank": rank, "graph": step.use_graph, "world": step.exchange.world_size, "gscale": step._gscale,
                  "launches": launches, "n_finish": len(summed), "loss": loss.item(), "step_t": opt.step_t.item(),
                  "families": sorted(step.families)}))
flat.close()
dist.destroy_process_group()
'''


def _local_gradient(rank):
    """What rank ``rank`` of the script adds to the exchange: the flat gradient of its batch and subset from a plain eager
    forward + backward of the same model and DropPath draws."""
    from fastvim_amd.hcs import ChannelSampler
    from fastvim_amd.losses import SoftTargetCrossEntropy
    m, flat, opt = _make()
    try:
        x = torch.randn(B, CHANNELS, SIZE, SIZE, generator=torch.Generator().manual_seed(1000 + rank)).cuda()
        tgt = torch.softmax(torch.randn(B, CLASSES, generator=torch.Generator().manual_seed(2000 + rank)), -1).cuda()
        sampler = ChannelSampler(CHANNELS)
        sampler.set([[0, 2], [1]][rank])
        torch.manual_seed(50 + rank)
        flat.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = SoftTargetCrossEntropy()(m(x, hcs=sampler), tgt)
        loss.backward()
        flat.finish_backward()
        torch.cuda.synchronize()
        return flat.grad_flat.detach().cpu().clone(), loss.item(), dict(flat.offsets)
    finally:
        flat.close()


def test_two_ranks_on_one_gpu(tmp_path, monkeypatch):
    """Two ranks share GPU 0 over gloo, a fresh child each, three buckets, each rank replaying the family of its own channel
    count: the gradient the optimizer graph reads after ``finish()`` is, bit for bit, the sum of the two ranks' own
    gradients (``cls_token``, complete only behind the last backward graph, included); both ranks end with identical
    weights, and those are the weights of ONE rank stepping on the mean of the two gradients."""
    import fastvim_amd.gemm as gemm_mod
    script = tmp_path / "channelvim_step_rank.py"
    script.write_text(_RANK_SCRIPT)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, str(r), "29571", str(tmp_path / f"rank{r}.pt")], env=env,
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
        assert o["launches"] == [0, 1, 2] and o["n_finish"] == 1 and o["families"] == [1, 2, 3]
    monkeypatch.setattr(gemm_mod, "FILL", False)
    (g0, l0, offsets), (g1, l1, _) = _local_gradient(0), _local_gradient(1)
    assert (a["loss"], b["loss"]) == (l0, l1) and l0 != l1
    ra, rb = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    want = g0 + g1                                                   # two fp32 terms: one rounding, whatever the order
    for name, n in (("cls_token", EMBED), ("pos_embed", P * EMBED), ("patch_embed.channel_embed.weight", CHANNELS * EMBED)):
        o = offsets[name]
        assert g0[o:o + n].abs().sum() > 0 and g1[o:o + n].abs().sum() > 0, name
        assert torch.equal(ra["grad"][o:o + n], want[o:o + n]), name
    assert torch.equal(ra["grad"], want) and torch.equal(rb["grad"], want)
    assert torch.isfinite(ra["params"]).all() and torch.equal(ra["params"], rb["params"])
    # one rank, the mean of the two gradients
    m, flat, opt = _make()
    try:
        flat.zero_grad()
        flat.grad_flat.copy_(want.cuda())
        opt.step(grad_scale=0.5)
        torch.cuda.synchronize()
        assert torch.equal(flat.param_flat.cpu(), ra["params"])
    finally:
        flat.close()
