"""The fused optimizer with parameter groups (layer-wise lr decay), global-norm gradient clipping and the skip of
non-finite steps -- csrc/optim.hip: grad_sumsq_kernel, adamw_flat_groups_kernel -- against the un-grouped kernel (bit for
bit), torch.optim.AdamW + torch.nn.utils.clip_grad_norm_, and fp64 norms."""
import copy
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def _tiny(img=(64, 64), depth=4, **kw):
    from fastvim_amd.fastvim import VisionMamba
    return VisionMamba(img_size=img, patch_size=16, depth=depth, embed_dim=32, channels=3, num_classes=10,
                       rms_norm=True, residual_in_fp32=True, fused_add_norm=True, final_pool_type="mean",
                       if_abs_pos_embed=True, drop_path_rate=0.0, **kw)


def _base_model(depth=4):
    torch.manual_seed(0)
    return _tiny(depth=depth).cuda().train()


def _seeded_grads(model, seed, scale=1.0):
    """One gradient per parameter NAME, from a seed (the same values whichever copy of the model they are written to)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return {n: torch.randn(p.shape, device="cuda", generator=g) * scale for n, p in model.named_parameters()}


def _write_grads(model, grads, factor=1.0):
    for n, p in model.named_parameters():
        if p.grad is None:
            p.grad = torch.empty_like(p)
        p.grad.copy_(grads[n] * factor)


def _state(flat, opt):
    out = {"param": flat.param_flat, "shadow": flat.shadow_flat, "exp_avg": opt.exp_avg, "exp_avg_sq": opt.exp_avg_sq,
           "step": opt.step_t}
    if opt.ema is not None:
        out["ema"] = opt.ema
    return {k: v.clone() for k, v in out.items()}


def _assert_same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("two_groups", [False, True])
def test_old_path_untouched_and_one_group_is_bit_identical(two_groups):
    """``FlatAdamW`` without the new arguments (fv_adamw_flat) and the grouped kernel with the same hyper-parameters as
    groups of lr_scale 1: every buffer bit-identical over several steps (the two kernels share the element update)."""
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    base = _base_model()
    ma, mb = copy.deepcopy(base), copy.deepcopy(base)
    fa, fb = FlatTrainingState(ma), FlatTrainingState(mb)
    nd = {n for n, p in ma.named_parameters() if p.ndim <= 1} if two_groups else set()
    oa = FlatAdamW(fa, ma, lr=3e-3, weight_decay=0.05, no_decay=nd, ema_decay=0.9)
    groups = [{"params": [p for n, p in mb.named_parameters() if n not in nd], "lr_scale": 1.0, "weight_decay": 0.05}]
    if nd:
        groups.append({"params": [p for n, p in mb.named_parameters() if n in nd], "lr_scale": 1.0, "weight_decay": 0.0})
    ob = FlatAdamW(fb, mb, lr=3e-3, weight_decay=0.05, param_groups=groups, ema_decay=0.9)
    assert not oa._grouped and oa.group_ids is None and ob._grouped and ob.partials is None
    for it in range(5):
        grads = _seeded_grads(base, 100 + it, scale=10.0 ** (it - 2))
        _write_grads(ma, grads); _write_grads(mb, grads)
        if it == 2:
            oa.set_lr(1e-3); ob.set_lr(1e-3)
        scale = 0.5 if it == 3 else 1.0
        oa.step(grad_scale=scale); ob.step(grad_scale=scale)
        _assert_same_state(_state(fa, oa), _state(fb, ob))
    assert oa.step_t.item() == 5.0
    fa.close(); fb.close()


def _chain_length(n):
    """d of the accuracy bound: the longest chain of dependent fp32 additions of the norm reduction over n elements, from
    the launch geometry the size query returns (csrc/optim.hip).  G workgroups, a trip of a workgroup covers 1024 float4
    and adds one term to each of a lane's 16 accumulators: ceil(n / 4 / (1024 G)) trips; then 4 (the 16 accumulators as a
    tree) + 6 (wave) + 2 (four waves) to the workgroup's partial, and 2 + 6 + 2 to finish the G <= 1024 partials."""
    from fastvim_amd import _lib as L
    G = int(L.lib().fv_grad_sumsq_blocks(ctypes.c_size_t(n)))
    return -(-(n // 4) // (G * 1024)) + (4 + 6 + 2) + (2 + 6 + 2), G


def _torch_side(m1, layer_decay, base_lr, weight_decay=0.05):
    from fastvim_amd.lr_decay import param_groups_lrd
    groups = param_groups_lrd(m1, weight_decay, no_weight_decay_list=m1.no_weight_decay(), layer_decay=layer_decay)
    for g in groups:
        g["lr"] = base_lr * g["lr_scale"]
    return torch.optim.AdamW(groups, lr=base_lr)


def _check_against(m1, m2, flat, o2, ema_ref):
    """The bounds of tests/test_model_gpu.py::test_flat_adamw_matches_torch_adamw."""
    p2 = dict(m2.named_parameters())
    for n, p in m1.named_parameters():
        assert (p - p2[n]).abs().max().item() <= 2e-6 * max(1.0, p.abs().max().item()), n
        assert (p2[n]._fv_shadow.float() - p2[n]).abs().max().item() <= 2.0 ** -8 * max(1e-3, p2[n].abs().max().item()), n
        off = flat.offsets[n]
        e = o2.ema[off:off + p.numel()].view_as(p)
        assert (e - ema_ref[n]).abs().max().item() <= 2e-6 * max(1.0, p.abs().max().item()), n


@pytest.mark.parametrize("layer_decay", [0.65, 0.75])
def test_groups_and_clipping_match_torch(layer_decay):
    """Optimizer only: identical seeded gradients go into ``p.grad`` of a deep copy (torch: clip_grad_norm_ + AdamW over
    the lr-decay groups at lr = base * lr_scale) and into the flat gradient (one fused step)."""
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    from fastvim_amd.lr_decay import param_groups_lrd
    base = _base_model(depth=6)
    m1, m2 = copy.deepcopy(base), copy.deepcopy(base)
    flat = FlatTrainingState(m2)
    max_norm = 3.0
    o1 = _torch_side(m1, layer_decay, 3e-3)
    groups = param_groups_lrd(m2, 0.05, no_weight_decay_list=m2.no_weight_decay(), layer_decay=layer_decay)
    assert len({g["lr_scale"] for g in groups}) >= 4
    o2 = FlatAdamW(flat, m2, lr=3e-3, param_groups=groups, max_grad_norm=max_norm, ema_decay=0.9)
    ema_ref = {n: p.detach().clone() for n, p in m1.named_parameters()}
    n_el = sum(p.numel() for p in base.parameters())
    d, _ = _chain_length(flat.grad_flat.numel())
    clipped = []
    for it, factor in enumerate((0.5, 2.0, 0.3, 5.0)):          # norm of the step's gradient ~ factor * max_norm
        grads = _seeded_grads(base, 7 + it, scale=factor * max_norm / n_el ** 0.5)
        _write_grads(m1, grads); _write_grads(m2, grads)
        assert all(torch.equal(p.grad, q.grad) for p, q in zip(m1.parameters(), m2.parameters()))
        if it == 2:
            for g in o1.param_groups:
                g["lr"] = 1e-3 * g["lr_scale"]
            o2.set_lr(1e-3)
        ref64 = torch.linalg.vector_norm(torch.cat([g.double().reshape(-1) for g in grads.values()])).item()
        tnorm = torch.nn.utils.clip_grad_norm_(list(m1.parameters()), max_norm).item()
        clipped.append(tnorm > max_norm)
        o1.step(); o2.step()
        st = o2.last_stats()
        print(f"step {it}: torch norm {tnorm:.9g} fused {st['total_norm']:.9g} fp64 {ref64:.9g} clip_coef {st['clip_coef']:.9g}")
        assert abs(st["total_norm"] - ref64) <= (d + 4) * 2.0 ** -24 * ref64
        assert abs(st["clip_coef"] - min(1.0, max_norm / (tnorm + 1e-6))) <= 1e-6 and st["finite"] and st["skipped_steps"] == 0
        for n, p in m1.named_parameters():
            ema_ref[n].mul_(0.9).add_(p.detach(), alpha=0.1)
    assert clipped == [False, True, False, True]                # both happen, by torch's own norms
    _check_against(m1, m2, flat, o2, ema_ref)
    assert o2.step_t.item() == 4.0
    flat.close()


def _lib_norm(g, grad_scale):
    """total_norm of the stats record for a raw gradient tensor, through the two launches of the C ABI (lr 0: nothing moves)."""
    from fastvim_amd import _lib as L
    n = g.numel()
    lib = L.lib()
    G = lib.fv_grad_sumsq_blocks(ctypes.c_size_t(n))
    dev = g.device
    z = lambda dt=torch.float32, k=n: torch.zeros(k, device=dev, dtype=dt)
    p, m, v, ids = z(), z(), z(), z(torch.uint8)
    table = torch.tensor([[1.0, 0.0]], device=dev)
    lr, step, partials, stats = z(k=1), z(k=1), torch.full((G,), float("nan"), device=dev), z(k=4)
    max_norm = torch.full((1,), 1.0, device=dev)
    st = L.stream_of(g)
    L.check(lib.fv_grad_sumsq_partials(L.ptr(g), L.ptr(partials), ctypes.c_size_t(n), st), "grad_sumsq_partials")
    L.check(lib.fv_adamw_flat_groups(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(None), L.ptr(None), L.ptr(ids),
                                     L.ptr(table), L.i32(1), L.ptr(lr), L.ptr(step), L.ptr(partials), L.i32(G),
                                     L.ptr(max_norm), L.ptr(stats), L.i32(0), ctypes.c_float(0.9), ctypes.c_float(0.999),
                                     ctypes.c_float(1e-8), ctypes.c_float(0.0), ctypes.c_float(grad_scale),
                                     ctypes.c_size_t(n), st), "adamw_flat_groups")
    torch.cuda.synchronize()
    assert step.item() == 1.0 and p.abs().max().item() == 0.0
    return stats.tolist(), G


# 8; one more float4 than three trips of one workgroup (not a multiple of the launch's coverage); ~7 M (FastVim-T); ~100 M
@pytest.mark.parametrize("n", [8, 4 * (3 * 1024 + 1), 7_000_004, 100_000_012])
@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
def test_norm_accuracy(n, grad_scale):
    """All terms are non-negative, so the relative error of the fp32 sum is at most about (d + 1) * 2**-24 with d the
    longest chain of dependent additions (the squares enter through an fma: no worse than rounding them first); the root
    halves it, root and scaling add one rounding each: |norm - ref| <= (d + 4) * 2**-24 * ref against fp64."""
    g_ = torch.Generator(device="cuda").manual_seed(n % 1000)
    mag = 10.0 ** (torch.rand(n, device="cuda", generator=g_) * 9.0 - 6.0)           # 1e-6 ... 1e3
    sign = torch.randint(0, 2, (n,), device="cuda", generator=g_).float() * 2 - 1
    g = (mag * sign).contiguous()
    (norm, coef, finite, _), G = _lib_norm(g, grad_scale)
    d, G_query = _chain_length(n)
    assert G_query == G
    ref = grad_scale * g.double().square().sum().sqrt().item()
    print(f"n {n} G {G} d {d}: norm {norm:.9g} ref {ref:.12g} rel err {abs(norm - ref) / ref:.3g} bound {(d + 4) * 2.0 ** -24:.3g}")
    assert finite == 1.0
    assert abs(norm - ref) <= (d + 4) * 2.0 ** -24 * ref
    assert abs(coef - min(1.0, 1.0 / (norm + 1e-6))) <= 1e-6 * coef


def test_power_of_two_scaling_is_exact():
    """Gradient 4 g with grad_scale 0.25 == gradient g with grad_scale 1: bit-identical parameters and clip_coef."""
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    from fastvim_amd.lr_decay import param_groups_lrd
    base = _base_model()
    runs = []
    for mult, scale in ((1.0, 1.0), (4.0, 0.25)):
        m = copy.deepcopy(base)
        flat = FlatTrainingState(m)
        groups = param_groups_lrd(m, 0.05, no_weight_decay_list=m.no_weight_decay(), layer_decay=0.75)
        opt = FlatAdamW(flat, m, lr=3e-3, param_groups=groups, max_grad_norm=1.0, ema_decay=0.9)
        coefs = []
        for it in range(3):
            _write_grads(m, _seeded_grads(base, 40 + it, scale=(0.001, 0.05, 1.0)[it]), factor=mult)
            opt.step(grad_scale=scale)
            coefs.append(opt.last_stats()["clip_coef"])
        runs.append((_state(flat, opt), coefs))
        flat.close()
    assert runs[0][1] == runs[1][1] and runs[0][1][0] == 1.0 and runs[0][1][2] < 1.0
    _assert_same_state(runs[0][0], runs[1][0])


def _opt_only_run(base, graph):
    """6 optimizer steps with groups + clipping, lr and max_grad_norm changed between steps; eager or one captured graph."""
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    from fastvim_amd.lr_decay import param_groups_lrd
    m = copy.deepcopy(base)
    flat = FlatTrainingState(m)
    groups = param_groups_lrd(m, 0.05, no_weight_decay_list=m.no_weight_decay(), layer_decay=0.65)
    opt = FlatAdamW(flat, m, lr=3e-3, param_groups=groups, max_grad_norm=1.0, ema_decay=0.99, skip_nonfinite=True)
    g = None
    if graph:
        snap = [(t, t.clone()) for t in [flat.param_flat, flat.shadow_flat] + [v for v in vars(opt).values() if torch.is_tensor(v)]]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            opt.step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        for t, saved in snap:
            t.copy_(saved)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            opt.step()
    stats = []
    for it in range(6):
        _write_grads(m, _seeded_grads(base, 60 + it, scale=0.02 * (it + 1)))
        opt.set_lr(3e-3 / (it + 1))
        opt.set_max_grad_norm(0.5 + 0.5 * (it % 3))
        g.replay() if graph else opt.step()
        stats.append(opt.last_stats())
    out = _state(flat, opt)
    flat.close()
    return out, stats


def test_deterministic_and_graph_replay_equals_eager():
    base = _base_model()
    e1, s1 = _opt_only_run(base, graph=False)
    e2, s2 = _opt_only_run(base, graph=False)
    _assert_same_state(e1, e2)
    assert s1 == s2
    r, s3 = _opt_only_run(base, graph=True)
    _assert_same_state(e1, r)
    assert s1 == s3 and e1["step"].item() == 6.0
    assert any(s["clip_coef"] < 1.0 for s in s1) and len({s["clip_coef"] for s in s1}) > 2


def test_segmented_train_step_replays_like_eager_with_groups_and_clipping():
    """Through SegmentedTrainStep (forward graph | backward graphs | optimizer graph, which now holds the norm launch and
    the grouped kernel), on the model of test_graph_replay_matches_eager_training[fastvim]."""
    from fastvim_amd.fastvim import VisionMamba
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    from fastvim_amd.losses import SoftTargetCrossEntropy
    from fastvim_amd.lr_decay import param_groups_lrd
    from fastvim_amd.pipeline import SegmentedTrainStep
    torch.manual_seed(0)
    base = VisionMamba(img_size=224, depth=4, embed_dim=192, num_classes=100, rms_norm=True, residual_in_fp32=True,
                       fused_add_norm=True, final_pool_type="mean", if_abs_pos_embed=True, drop_path_rate=0.0).cuda().train()
    x = torch.randn(16, 3, 224, 224, device="cuda")
    tgt = torch.softmax(torch.randn(16, 100, device="cuda"), -1)
    crit = SoftTargetCrossEntropy()

    def make():
        m = copy.deepcopy(base)
        flat = FlatTrainingState(m)
        groups = param_groups_lrd(m, 0.05, no_weight_decay_list=m.no_weight_decay(), layer_decay=0.75)
        return m, flat, FlatAdamW(flat, m, lr=1e-3, param_groups=groups, max_grad_norm=1.0, ema_decay=0.999)

    m0, f0, o0 = make()                 # the size of this model's gradient: max_grad_norm is set around it, both sides
    f0.zero_grad()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        crit(m0(x), tgt).backward()
    f0.finish_backward()
    norm0 = torch.linalg.vector_norm(f0.grad_flat).item()
    f0.close()
    sched = [(1e-3, 4.0 * norm0), (8e-4, 0.5 * norm0), (6e-4, 0.25 * norm0), (4e-4, 8.0 * norm0), (2e-4, 0.1 * norm0),
             (1e-4, norm0)]
    m1, f1, o1 = make()
    ref, ref_stats = [], []
    for lr, mn in sched:
        o1.set_lr(lr); o1.set_max_grad_norm(mn)
        f1.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = crit(m1(x), tgt)
        loss.backward()
        o1.step()
        ref.append(loss.item()); ref_stats.append(o1.last_stats())
    m2, f2, o2 = make()
    seg = SegmentedTrainStep(m2, f2, o2, crit, x, tgt, n_segments=3, use_graph=True, warmup=2)
    assert seg.graphs is not None
    got, got_stats = [], []
    for lr, mn in sched:
        o2.set_lr(lr); o2.set_max_grad_norm(mn)
        got.append(seg.step().item()); got_stats.append(o2.last_stats())
    torch.cuda.synchronize()
    assert got == ref and got_stats == ref_stats, (got, ref)
    assert ref_stats[0]["clip_coef"] == 1.0 and ref_stats[1]["clip_coef"] < 1.0       # both clipped and unclipped steps
    _assert_same_state(_state(f1, o1), _state(f2, o2))
    assert o2.step_t.item() == 6.0 and o2.last_stats()["skipped_steps"] == 0
    f1.close(); f2.close()


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_skip_nonfinite(bad):
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    from fastvim_amd.lr_decay import param_groups_lrd
    base = _base_model()

    def make():
        m = copy.deepcopy(base)
        flat = FlatTrainingState(m)
        groups = param_groups_lrd(m, 0.05, no_weight_decay_list=m.no_weight_decay(), layer_decay=0.75)
        return m, flat, FlatAdamW(flat, m, lr=3e-3, param_groups=groups, max_grad_norm=1.0, ema_decay=0.9, skip_nonfinite=True)

    def good_step(m, opt, it):
        _write_grads(m, _seeded_grads(base, 80 + it, scale=0.05))
        opt.step()

    ma, fa, oa = make()
    mb, fb, ob = make()
    good_step(ma, oa, 0); good_step(mb, ob, 0)
    before = _state(fa, oa)
    _write_grads(ma, _seeded_grads(base, 99, scale=0.05))
    fa.grad_flat[fa.offsets["layers.1.mixer.in_proj.weight"] + 5] = bad
    oa.step()
    st = oa.last_stats()
    assert not st["finite"] and st["skipped_steps"] == 1
    _assert_same_state(before, _state(fa, oa))                  # parameters, moments, EMA, shadow, step count: untouched
    assert oa.step_t.item() == 1.0
    for it in (1, 2):
        good_step(ma, oa, it); good_step(mb, ob, it)
    _assert_same_state(_state(fa, oa), _state(fb, ob))          # as if the bad step had never been seen
    assert oa.last_stats() == {**ob.last_stats(), "skipped_steps": 1} and oa.step_t.item() == 3.0
    # without the skip the same gradient is NOT ignored (the norm is non-finite and says so)
    mc, fc, oc = make()
    oc.skip_nonfinite = False
    _write_grads(mc, _seeded_grads(base, 99, scale=0.05))
    fc.grad_flat[0] = bad
    oc.step()
    assert not oc.last_stats()["finite"] and oc.last_stats()["skipped_steps"] == 0 and oc.step_t.item() == 1.0
    fa.close(); fb.close(); fc.close()


def test_end_to_end_training_matches_torch():
    """Tiny VisionMamba, 4 training steps with lr-decay groups and a max_grad_norm low enough to clip, against the deep
    copy trained by torch AdamW + clip_grad_norm_ -- in the manner and at the tolerance of
    tests/test_model_gpu.py::test_flat_adamw_matches_torch_adamw."""
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    from fastvim_amd.lr_decay import param_groups_lrd
    torch.manual_seed(0)
    m1 = _tiny().cuda().train()
    m2 = copy.deepcopy(m1)
    flat = FlatTrainingState(m2)
    x = torch.randn(4, 3, 64, 64, device="cuda")
    m1(x).float().square().mean().backward()
    flat.finish_backward()          # (the flat state switched the wrappers to deferred reductions process-wide)
    norm0 = torch.linalg.vector_norm(torch.cat([p.grad.reshape(-1) for p in m1.parameters()])).item()
    max_norm = 0.5 * norm0
    o1 = _torch_side(m1, 0.75, 3e-3)
    groups = param_groups_lrd(m2, 0.05, no_weight_decay_list=m2.no_weight_decay(), layer_decay=0.75)
    o2 = FlatAdamW(flat, m2, lr=3e-3, param_groups=groups, max_grad_norm=max_norm, ema_decay=0.9)
    ema_ref = {n: p.detach().clone() for n, p in m1.named_parameters()}
    clipped = []
    for it in range(4):
        for m, zero in ((m1, lambda: m1.zero_grad(set_to_none=True)), (m2, flat.zero_grad)):
            zero()
            m(x).float().square().mean().backward()
        flat.finish_backward()
        if it == 2:
            for g in o1.param_groups:
                g["lr"] = 1e-3 * g["lr_scale"]
            o2.set_lr(1e-3)
        tnorm = torch.nn.utils.clip_grad_norm_(list(m1.parameters()), max_norm).item()
        clipped.append(tnorm > max_norm)
        o1.step(); o2.step()
        st = o2.last_stats()
        print(f"step {it}: torch norm {tnorm:.7g} fused {st['total_norm']:.7g} clip_coef {st['clip_coef']:.6g}")
        # (a loose sanity bound on purpose: the two sides' gradients come from two separate bf16 backward passes, so their
        # norms differ by more than the reduction's rounding; the tight bound on the norm is test_norm_accuracy's and
        # test_groups_and_clipping_match_torch's, where both sides start from bit-identical gradients)
        assert abs(st["total_norm"] - tnorm) <= 1e-4 * tnorm
        for n, p in m1.named_parameters():
            ema_ref[n].mul_(0.9).add_(p.detach(), alpha=0.1)
    assert clipped[0]             # the first step clips, by torch's own norm (later gradients shrink as the loss falls)
    _check_against(m1, m2, flat, o2, ema_ref)
    flat.close()
