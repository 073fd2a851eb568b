"""``FlatAdamW.set_weight_decay``: the scheduled weight decay of the cell-imaging recipes as a write into the grouped kernel's
device table.  A step after ``set_weight_decay(w)`` against the step of an optimizer CONSTRUCTED with ``weight_decay=w``, bit
for bit; a captured optimizer graph replayed under three values; the no-decay rows; the ``state_dict`` round trip; and what
an optimizer built without any of it does (``fv_adamw_flat``, and an error that names the constructor argument)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

WD0 = 0.05


def _make(seed=3, **kw):
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    from fastvim_amd.models_channel_mamba import VisionMamba
    torch.manual_seed(seed)
    m = VisionMamba(img_size=32, patch_size=16, channels=3, depth=2, embed_dim=32, num_classes=10, rms_norm=True,
                    residual_in_fp32=True, fused_add_norm=True, if_cls_token=True, if_abs_pos_embed=True).cuda().train()
    flat = FlatTrainingState(m)
    nd = {n for n, p in m.named_parameters() if p.ndim <= 1 or n.endswith(".bias") or n in m.no_weight_decay()}
    kw.setdefault("weight_decay", WD0)
    return m, flat, FlatAdamW(flat, m, lr=3e-3, no_decay=nd, ema_decay=0.9, **kw), nd


def _grad(flat, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    flat.grad_flat.copy_(0.1 * torch.randn(flat.grad_flat.numel(), device="cuda", generator=g))


def _state(flat, opt):
    return [t.clone() for t in (flat.param_flat, flat.shadow_flat, opt.exp_avg, opt.exp_avg_sq, opt.ema, opt.step_t)]


def _put(flat, opt, state):
    for dst, src in zip((flat.param_flat, flat.shadow_flat, opt.exp_avg, opt.exp_avg_sq, opt.ema, opt.step_t), state):
        dst.copy_(src)


def _same(a, b):
    names = ("param_flat", "shadow_flat", "exp_avg", "exp_avg_sq", "ema", "step_t")
    for n, x, y in zip(names, a, b):
        assert torch.equal(x, y), n


def test_step_after_set_weight_decay_equals_an_optimizer_constructed_with_it():
    w = 0.31
    m1, f1, o1, nd = _make(scheduled_weight_decay=True)
    m2, f2, o2, _ = _make(scheduled_weight_decay=True, weight_decay=w)
    m3, f3, o3, _ = _make(scheduled_weight_decay=True)                     # the control: the constructor's value
    try:
        assert torch.equal(f1.param_flat, f2.param_flat)
        o1.set_weight_decay(w)
        assert torch.equal(o1.group_table, o2.group_table) and not torch.equal(o1.group_table, o3.group_table)
        for it in range(2):
            for f, o in ((f1, o1), (f2, o2), (f3, o3)):
                _grad(f, 10 + it)
                o.step()
        torch.cuda.synchronize()
        _same(_state(f1, o1), _state(f2, o2))
        assert not torch.equal(f1.param_flat, f3.param_flat)                # the value matters to the update
        # the parameters that are not decayed moved exactly as under the constructor's value
        for name in sorted(nd)[:8]:
            o, k = f1.offsets[name], dict(m1.named_parameters())[name].numel()
            assert torch.equal(f1.param_flat[o:o + k], f3.param_flat[o:o + k]), name
    finally:
        f3.close(); f2.close(); f1.close()


def test_captured_optimizer_graph_replays_with_the_scheduled_value():
    m1, f1, o1, _ = _make(scheduled_weight_decay=True)
    try:
        _grad(f1, 1)
        start = _state(f1, o1)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            o1.step()                                                       # warm-up outside the capture ...
        torch.cuda.current_stream().wait_stream(side)
        _put(f1, o1, start)                                                 # ... undone
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            o1.step()
        _put(f1, o1, start)                                                 # (capture runs nothing; be explicit anyway)
        finals = []
        for it, w in enumerate((0.1, 0.25, 0.4)):
            _grad(f1, 20 + it)
            before = _state(f1, o1)
            o1.set_weight_decay(w)
            graph.replay()
            torch.cuda.synchronize()
            after = _state(f1, o1)
            # a fresh optimizer constructed with this value, put into the same state, stepping eagerly
            m2, f2, o2, _ = _make(scheduled_weight_decay=True, weight_decay=w)
            try:
                _put(f2, o2, before)
                _grad(f2, 20 + it)
                o2.step()
                torch.cuda.synchronize()
                _same(after, _state(f2, o2))
            finally:
                f2.close()
            finals.append(after[0])
        assert o1.step_t.item() == 3.0 and not torch.equal(finals[0], finals[1])
    finally:
        f1.close()


def test_no_decay_rows_stay_zero_and_state_dict_round_trips():
    import numpy as np
    m1, f1, o1, nd = _make(scheduled_weight_decay=True)
    m2, f2, o2, _ = _make(scheduled_weight_decay=True)
    try:
        o1.set_weight_decay(0.3)
        sd = o1.state_dict()
        groups = sd["param_groups"]
        assert set(groups) == set(f1.names)
        for name, (scale, wd) in groups.items():
            assert scale == 1.0 and wd == (0.0 if name in nd else float(np.float32(0.3))), name
        assert "cls_token" in nd and "pos_embed" in nd and any(n not in nd for n in groups)
        assert sd["weight_decay"] == WD0                                    # the constructor's value, as before
        o2.load_state_dict(sd)
        assert torch.equal(o2.group_table, o1.group_table) and torch.equal(o2.group_ids, o1.group_ids)
        assert o2.state_dict()["param_groups"] == groups
        # the loaded optimizer goes on with the schedule: the same rows, the same step
        for o in (o1, o2):
            o.set_weight_decay(0.2)
        assert torch.equal(o2.group_table, o1.group_table)
        assert all(wd == 0.0 for n, (_, wd) in o2.state_dict()["param_groups"].items() if n in nd)
        for f, o in ((f1, o1), (f2, o2)):
            _grad(f, 5)
            o.step()
        torch.cuda.synchronize()
        _same(_state(f1, o1), _state(f2, o2))
    finally:
        f2.close(); f1.close()


def test_param_groups_rows_take_the_value_too():
    """With explicit groups every decayed row takes the scheduled value and keeps its lr_scale; a group built with
    ``weight_decay=0`` is a no-decay group."""
    m, f, _, nd = _make()
    from fastvim_amd.flat import FlatAdamW
    try:
        named = dict(m.named_parameters())
        decayed = [n for n in f.names if n not in nd]
        groups = [{"params": [named[n] for n in decayed[:2]], "lr_scale": 0.5, "weight_decay": 0.05},
                  {"params": [named[n] for n in decayed[2:]], "lr_scale": 1.0, "weight_decay": 0.1},
                  {"params": [named[n] for n in f.names if n in nd], "lr_scale": 1.0, "weight_decay": 0.0}]
        opt = FlatAdamW(f, m, lr=1e-3, param_groups=groups)
        opt.set_weight_decay(0.4)
        assert opt.group_table.tolist() == [[0.5, pytest.approx(0.4)], [1.0, pytest.approx(0.4)], [1.0, 0.0]]
        assert not opt._group_table_full[3:].any()
    finally:
        f.close()


def test_an_ungrouped_optimizer_launches_what_it_launched_and_refuses_the_schedule(monkeypatch):
    import fastvim_amd.flat as flat_mod
    calls = []
    real = flat_mod.L.lib()

    class Spy:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(real, name)
    m, f, opt, _ = _make()
    m2, f2, sched, _ = _make(scheduled_weight_decay=True)
    try:
        assert opt._grouped is False and opt.group_table is None and opt.decay_mask is not None
        with pytest.raises(RuntimeError, match="scheduled_weight_decay=True"):
            opt.set_weight_decay(0.2)
        assert opt.state_dict()["param_groups"] is None
        monkeypatch.setattr(flat_mod.L, "lib", lambda: Spy())
        _grad(f, 2)
        opt.step()
        assert "fv_adamw_flat" in calls and "fv_adamw_flat_groups" not in calls and "fv_grad_sumsq_partials" not in calls
        del calls[:]
        _grad(f2, 2)
        sched.step()
        assert "fv_adamw_flat_groups" in calls and "fv_adamw_flat" not in calls and "fv_grad_sumsq_partials" not in calls
        torch.cuda.synchronize()
        # ... and the two kernels compute the same update from the same value
        _same(_state(f, opt), _state(f2, sched))
    finally:
        f2.close(); f.close()
