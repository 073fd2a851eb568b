"""The linear-probe step (fastvim_amd/linear_probe.py) on a 2-layer FastVim, batch 8, under bf16 autocast and in fp32:
graph replay against eager, construction side effects, the frozen backbone, the head against an fp64 restatement, the
no-library-GEMM rule, frozen shadows, and the collectives over a one-rank RCCL group.

Reference comparison: the model's own ``no_grad`` features go through fp64 BatchNorm -> linear -> cross-entropy -> SGD
(momentum 0.9) for 4 steps; tolerance 4 x what the same composition in fp32 torch on the CPU deviates from fp64, measured
in the test.  For bf16 the xhat and weight inputs of the head GEMM are storage-rounded in both restatements.
"""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, MOM, STEPS = 0.1, 0.9, 4
AMPS = pytest.mark.parametrize("amp", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])


def _model():
    from fastvim_amd.fastvim import VisionMamba
    from fastvim_amd.linear_probe import attach_probe_head
    torch.manual_seed(0)
    m = VisionMamba(img_size=64, depth=2, embed_dim=192, num_classes=10, rms_norm=True, residual_in_fp32=True,
                    fused_add_norm=True, final_pool_type="mean", if_abs_pos_embed=True)
    return attach_probe_head(m).cuda().train()


def _batch():
    g = torch.Generator().manual_seed(1)
    return torch.randn(8, 3, 64, 64, generator=g).cuda(), torch.randint(0, 10, (8,), generator=g).cuda()


def _state(m, opt):
    bn = m.head[0]
    return {"weight": m.head[1].weight.detach().clone(), "bias": m.head[1].bias.detach().clone(),
            "shadow": m.head[1].weight._fv_shadow.clone(), "momentum": opt.momentum_buf.clone(),
            "running_mean": bn.running_mean.clone(), "running_var": bn.running_var.clone(),
            "num_batches_tracked": bn.num_batches_tracked.clone()}


def _train(amp, use_graph, shadows=True):
    """A fresh model, 4 steps -> (losses, state after, state before construction, state after construction, model)."""
    from fastvim_amd.flat import FlatSGD, FlatTrainingState
    from fastvim_amd.linear_probe import LinearProbeStep, freeze_shadows
    m = _model()
    if shadows:
        freeze_shadows(m)
    x, labels = _batch()
    frozen = {n: p.detach().clone() for n, p in m.named_parameters() if not p.requires_grad}
    flat = FlatTrainingState(m)
    opt = FlatSGD(flat, m, lr=LR, momentum=MOM)
    before = _state(m, opt)
    step = LinearProbeStep(m, flat, opt, x, labels, amp_dtype=amp, use_graph=use_graph)
    torch.cuda.synchronize()
    built = _state(m, opt)
    assert step.use_graph == use_graph
    losses = []
    for _ in range(STEPS):
        losses.append(step.step().clone())
    torch.cuda.synchronize()
    after = _state(m, opt)
    flat.close()
    return torch.stack(losses), after, before, built, m, frozen


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


@AMPS
def test_graph_replay_equals_eager_and_construction_changes_nothing(amp):
    lg, sg, before, built, m, frozen = _train(amp, True)
    le, se, _, _, _, _ = _train(amp, False)
    lg2, sg2, _, _, _, _ = _train(amp, True)
    assert _same(before, built), "constructing the step object must leave every buffer as found"
    assert int(before["num_batches_tracked"]) == 0 and int(sg["num_batches_tracked"]) == STEPS
    assert torch.equal(lg, le) and _same(sg, se), (lg.tolist(), le.tolist())
    assert torch.equal(lg, lg2) and _same(sg, sg2)
    assert torch.isfinite(lg).all() and lg[-1] < lg[0]                       # the head learns the fixed batch
    assert not torch.equal(sg["weight"], before["weight"]) and torch.equal(sg["shadow"], sg["weight"].to(torch.bfloat16))
    # the frozen backbone: bit-unchanged, and no gradient was ever allocated for it
    for n, p in m.named_parameters():
        if not p.requires_grad:
            assert torch.equal(p, frozen[n]) and p.grad is None, n
    assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == ["head.1.bias", "head.1.weight"]


def _restate(feats, w0, b0, labels, dt, round_bf16):
    """BatchNorm -> linear -> cross-entropy -> SGD(momentum) on fixed features, in ``dt`` on the CPU."""
    r = (lambda t: t.to(torch.bfloat16).to(dt)) if round_bf16 else (lambda t: t)
    x = feats.to(dt)
    w, b = w0.to(dt).clone(), b0.to(dt).clone()
    rm, rv = torch.zeros(x.shape[1], dtype=dt), torch.ones(x.shape[1], dtype=dt)
    mw, mb = torch.zeros_like(w), torch.zeros_like(b)
    losses = []
    for _ in range(STEPS):
        xh = r(F.batch_norm(x, rm, rv, None, None, True, 0.1, 1e-6))
        wl, bl = w.clone().requires_grad_(), b.clone().requires_grad_()
        # (the GEMM reads the rounded weight, the gradient belongs to the master: a straight-through rounding)
        logits = xh @ (wl + (r(wl.detach()) - wl.detach())).t() + bl
        loss = F.cross_entropy(logits, labels)
        gw, gb = torch.autograd.grad(loss, (wl, bl))
        mw, mb = MOM * mw + gw, MOM * mb + gb
        w, b = w - LR * mw, b - LR * mb
        losses.append(loss.detach())
    return {"loss": torch.stack(losses), "weight": w, "bias": b, "running_mean": rm, "running_var": rv}


@AMPS
def test_head_against_fp64_restatement(amp):
    from fastvim_amd.flat import FlatSGD, FlatTrainingState
    from fastvim_amd.linear_probe import LinearProbeStep
    m = _model()
    # the model's default drop_path_rate is 0.1: in training mode every forward draws its own DropPath masks, so the
    # features would change from step to step.  The backbone is frozen: it runs in eval mode here, the head (its
    # BatchNorm takes batch statistics) in training mode -- then the step's features are the ones computed below
    m.eval()
    m.head.train()
    x, labels = _batch()
    with torch.no_grad(), torch.autocast("cuda", dtype=amp, enabled=amp != torch.float32):
        feats = m.forward_features(x)
        again = m.forward_features(x)
    assert feats.dtype == amp and feats.shape == (8, 192) and torch.equal(feats, again)
    w0, b0 = m.head[1].weight.detach().cpu().clone(), m.head[1].bias.detach().cpu().clone()
    with FlatTrainingState(m) as flat:
        opt = FlatSGD(flat, m, lr=LR, momentum=MOM)
        step = LinearProbeStep(m, flat, opt, x, labels, amp_dtype=amp)
        losses = torch.stack([step.step().clone() for _ in range(STEPS)])
        torch.cuda.synchronize()
        got = {"loss": losses, "weight": m.head[1].weight.detach(), "bias": m.head[1].bias.detach(),
               "running_mean": m.head[0].running_mean, "running_var": m.head[0].running_var}
        got = {k: v.cpu().clone() for k, v in got.items()}
    rb = amp == torch.bfloat16
    ref64 = _restate(feats.float().cpu(), w0, b0, labels.cpu(), torch.float64, rb)
    ref32 = _restate(feats.float().cpu(), w0, b0, labels.cpu(), torch.float32, rb)
    for k in ref64:
        err = (got[k].double() - ref64[k]).abs().max().item()
        base = (ref32[k].double() - ref64[k]).abs().max().item()
        print(f"{k}: max err {err:.3e}, fp32 torch on the CPU {base:.3e}, allowed {4 * base:.3e}")
    for k in ref64:
        err = (got[k].double() - ref64[k]).abs().max().item()
        base = (ref32[k].double() - ref64[k]).abs().max().item()
        assert err <= 4 * base, (k, err, base)


_GEMM_ENTRY_POINTS = ("bmm", "baddbmm", "matmul", "mm", "addmm", "einsum")


def _trap_library_calls(mp, hits):
    """Every torch matmul / linear / conv / batch-norm entry point raises (own copy of the mechanism of
    tests/test_model_gpu.py::test_training_step_calls_no_library_gemm, plus the batch-norm entries)."""
    def trap(name):
        def f(*a, **k):
            hits.append(name)
            raise AssertionError(f"library call {name} on the product path")
        return f

    for mod, name in ([(torch, n) for n in _GEMM_ENTRY_POINTS] + [(torch, "batch_norm"), (torch, "native_batch_norm")] +
                      [(F, "linear"), (F, "conv2d"), (F, "conv3d"), (F, "batch_norm"), (torch.Tensor, "__matmul__"),
                       (torch.Tensor, "matmul"), (torch.Tensor, "mm"), (torch.Tensor, "bmm"), (torch.Tensor, "baddbmm_")]):
        mp.setattr(mod, name, trap(name))


@AMPS
def test_probe_step_and_eval_forward_call_no_library_gemm_or_batch_norm(monkeypatch, amp):
    from fastvim_amd.flat import FlatSGD, FlatTrainingState
    from fastvim_amd.linear_probe import LinearProbeStep
    m = _model()
    x, labels = _batch()
    hits = []
    with FlatTrainingState(m) as flat:
        opt = FlatSGD(flat, m, lr=LR, momentum=MOM)
        with monkeypatch.context() as mp:
            _trap_library_calls(mp, hits)
            step = LinearProbeStep(m, flat, opt, x, labels, amp_dtype=amp, use_graph=False)
            loss = step.step()
            m.eval()
            with torch.no_grad(), torch.autocast("cuda", dtype=amp, enabled=amp != torch.float32):
                logits = m(x)
            torch.cuda.synchronize()
            assert not hits and torch.isfinite(loss) and torch.isfinite(logits).all() and logits.shape == (8, 10)
            assert flat.grad_flat.abs().max() > 0
    with pytest.raises(AssertionError, match="library call"):          # the trap itself works: torch's module trips it
        with monkeypatch.context() as mp:
            _trap_library_calls(mp, hits)
            torch.nn.BatchNorm1d(192, affine=False).cuda()(torch.randn(8, 192, device="cuda"))


def test_freeze_shadows_stops_the_weight_casts_and_keeps_the_logits(monkeypatch):
    """Without frozen shadows every projection weight falls through ``_shadow`` to a cast on every forward; with them none
    does, and the logits are bit-identical."""
    import fastvim_amd.fastvim as fv
    import fastvim_amd.linear_probe as lp
    import fastvim_amd.mamba_simple_faster as msf
    m = _model().eval()
    x, _ = _batch()
    casts = []
    real = msf._shadow

    def counting(w, cdt):
        out = real(w, cdt)
        if w.dtype != cdt and out is not getattr(w, "_fv_shadow", None):
            casts.append(tuple(w.shape))              # a fall-through: a weight-sized tensor in the compute dtype was made
        return out

    for mod in (msf, fv, lp):
        monkeypatch.setattr(mod, "_shadow", counting)

    def forward():
        del casts[:]
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return m(x).clone(), len(casts)

    y0, n0 = forward()
    assert n0 >= 2 * 2 + 2                             # per block in_proj and out_proj; the patch embedding; the head
    buf = lp.freeze_shadows(m)
    assert buf.dtype == torch.bfloat16
    y1, n1 = forward()
    assert n1 == 1, casts                              # only the (trainable) head weight is left: it belongs to a flat state
    assert torch.equal(y0, y1)
    # a later load_state_dict is still caught by the version check: the copy is re-cast in place, not bypassed
    sd = {k: (v * 1.5 if k.endswith("in_proj.weight") else v) for k, v in m.state_dict().items()}
    m.load_state_dict(sd)
    y2, n2 = forward()
    assert n2 == 1 and not torch.equal(y1, y2)
    w = m.layers[0].mixer.in_proj.weight
    assert torch.equal(w._fv_shadow, w.detach().to(torch.bfloat16))


_RCCL_SCRIPT = r'''
import os, sys, json
sys.path.insert(0, sys.argv[1])
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
import torch, torch.distributed as dist
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_linear_probe_gpu as T
from fastvim_amd.flat import FlatSGD, FlatTrainingState
from fastvim_amd.linear_probe import LinearProbeStep
torch.cuda.set_device(0)
dist.init_process_group("nccl", init_method="tcp://127.0.0.1:" + sys.argv[2], rank=0, world_size=1)
def run(sync):
    m = T._model()
    x, labels = T._batch()
    flat = FlatTrainingState(m)
    opt = FlatSGD(flat, m, lr=T.LR, momentum=T.MOM)
    step = LinearProbeStep(m, flat, opt, x, labels, use_graph=True, warmup=1, sync=sync)
    losses = [step.step().item() for _ in range(T.STEPS)]
    torch.cuda.synchronize()
    out = (losses, flat.param_flat.double().abs().sum().item(), m.head[0].running_var.double().sum().item(),
           int(m.head[0].num_batches_tracked), len(step.graphs))
    flat.close()
    return out
a = run(True)
b = run(False)
dist.destroy_process_group()
print(json.dumps({"synced": a, "plain": b}))
'''


def test_collectives_over_a_one_rank_rccl_group(tmp_path):
    """The multi-rank form of the step -- three graphs with the table all-gather and the gradient all-reduce between
    them -- over the real RCCL backend with one rank, where both collectives are the identity: losses, parameters and
    running statistics equal the single-graph step's bit for bit."""
    script = tmp_path / "probe_rccl_one_rank.py"
    script.write_text(_RCCL_SCRIPT)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(script), ROOT, "29563"], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    a, b = out["synced"], out["plain"]
    assert a[:4] == b[:4] and all(v == v for v in a[0]), out
    assert a[3] == 4 and a[4] == 3 and b[4] == 1
