"""CPU-side checks of the grouped / clipping fused optimizer (fastvim_amd/flat.py): the pure builder of the group bytes and
the table, the new keys of the optimizer's state dictionary, and the host-side size query of the norm launch."""
import ctypes

import pytest
import torch


def _layout():
    # three parameters at offsets that are multiples of 8 (FlatTrainingState pads every parameter to 8 elements)
    names = ["a", "b", "c"]
    sizes = {"a": 5, "b": 16, "c": 3}
    offsets = {"a": 0, "b": 8, "c": 24}
    return names, offsets, sizes, 32


def test_group_bytes_follow_the_offsets():
    from fastvim_amd.flat import build_group_map
    names, offsets, sizes, total = _layout()
    ids, table, per_name = build_group_map(names, offsets, sizes, total, [
        {"params": ["c"], "lr_scale": 0.5, "weight_decay": 0.0},
        {"params": ["a"], "lr_scale": 0.25},
        {"params": ["b"], "weight_decay": 0.1}], default_weight_decay=0.05)
    assert table == [(0.5, 0.0), (0.25, 0.05), (1.0, 0.1)]                     # first-seen order, defaults filled in
    exp = [1] * 5 + [0] * 3 + [2] * 16 + [0] * 3 + [0] * 5                     # padding = row 0 (and "c" is row 0 itself)
    assert ids.dtype == torch.uint8 and ids.tolist() == exp
    assert per_name == {"c": (0.5, 0.0), "a": (0.25, 0.05), "b": (1.0, 0.1)}


def test_equal_groups_are_merged():
    from fastvim_amd.flat import build_group_map, groups_from_named
    names, offsets, sizes, total = _layout()
    ids, table, per_name = build_group_map(names, offsets, sizes, total, [
        {"params": ["a"], "lr_scale": 0.5, "weight_decay": 0.05}, {"params": ["b"], "lr_scale": 1.0, "weight_decay": 0.05},
        {"params": ["c"], "lr_scale": 0.5, "weight_decay": 0.05}])
    assert table == [(0.5, 0.05), (1.0, 0.05)]
    assert ids[:5].tolist() == [0] * 5 and ids[8:24].tolist() == [1] * 16 and ids[24:27].tolist() == [0] * 3
    back = groups_from_named(per_name)                                           # the state-dict form and back
    assert back == [{"lr_scale": 0.5, "weight_decay": 0.05, "params": ["a", "c"]},
                    {"lr_scale": 1.0, "weight_decay": 0.05, "params": ["b"]}]
    ids2, table2, per_name2 = build_group_map(names, offsets, sizes, total, back)
    assert torch.equal(ids, ids2) and table == table2 and per_name == per_name2


def test_construction_errors():
    from fastvim_amd.flat import build_group_map
    names, offsets, sizes, total = _layout()
    with pytest.raises(ValueError, match="more than one group"):
        build_group_map(names, offsets, sizes, total, [{"params": ["a", "b"]}, {"params": ["c", "a"], "lr_scale": 0.5}])
    with pytest.raises(ValueError, match="in no group"):
        build_group_map(names, offsets, sizes, total, [{"params": ["a", "b"]}])
    with pytest.raises(ValueError, match="not a trainable parameter"):
        build_group_map(names, offsets, sizes, total, [{"params": ["a", "b", "c", "d"]}])


def test_256_groups_accepted_257_refused():
    from fastvim_amd.flat import build_group_map

    def layout(k):
        names = [f"p{i}" for i in range(k)]
        return names, {n: 8 * i for i, n in enumerate(names)}, {n: 8 for n in names}, 8 * k

    names, offsets, sizes, total = layout(256)
    ids, table, _ = build_group_map(names, offsets, sizes, total,
                                    [{"params": [n], "lr_scale": 1.0 / (i + 1)} for i, n in enumerate(names)])
    assert len(table) == 256 and ids[-1].item() == 255 and ids[::8].tolist() == list(range(256))
    names, offsets, sizes, total = layout(257)
    with pytest.raises(ValueError, match="more than 256"):
        build_group_map(names, offsets, sizes, total, [{"params": [n], "lr_scale": 1.0 / (i + 1)} for i, n in enumerate(names)])
    # 257 groups of which two are equal are 256 rows
    gs = [{"params": [n], "lr_scale": 1.0 / (min(i, 255) + 1)} for i, n in enumerate(names)]
    assert len(build_group_map(names, offsets, sizes, total, gs)[1]) == 256


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.patch_embed = torch.nn.Linear(6, 4)
        self.layers = torch.nn.ModuleList(torch.nn.Linear(4, 4) for _ in range(3))
        self.head = torch.nn.Linear(4, 2)


def _cpu_optimizer(**kw):
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    from fastvim_amd.lr_decay import param_groups_lrd
    torch.manual_seed(0)
    m = _Net()
    flat = FlatTrainingState(m)
    groups = param_groups_lrd(m, 0.05, layer_decay=0.5)
    return m, flat, FlatAdamW(flat, m, lr=1e-3, param_groups=groups, ema_decay=0.99, **kw)


def test_state_dict_round_trip_and_old_dictionaries():
    """The optimizer object holds only tensors until ``step()``: it is built on the CPU here."""
    from fastvim_amd.flat import FlatAdamW
    m, flat, opt = _cpu_optimizer(max_grad_norm=3.0, skip_nonfinite=True)
    assert opt.group_table.shape == (6, 2)       # 10 groups of param_groups_lrd, 3 distinct scales x (decayed, not) rows
    sd = opt.state_dict()
    pg = sd["param_groups"]
    assert set(pg) == set(flat.names) and sd["max_grad_norm"] == 3.0 and sd["skipped_steps"] == 0
    # L = 4: layer id 0 at 0.5 ** 2, ids 1 .. 4 at 0.5 ** 2, 1, 1, 0
    assert pg["patch_embed.weight"] == (0.25, pytest.approx(0.05)) and pg["patch_embed.bias"] == (0.25, 0.0)
    assert pg["layers.0.weight"][0] == 0.25 and pg["layers.1.weight"][0] == 0.5 and pg["layers.2.bias"] == (0.5, 0.0)
    assert pg["head.weight"] == (1.0, pytest.approx(0.05))
    # the table is writable between steps, and what is written is what is saved
    opt.group_table[:, 0] *= 0.5
    opt.set_max_grad_norm(1.5)
    opt.stats[3] = 4.0
    sd = opt.state_dict()
    assert sd["param_groups"]["head.weight"][0] == 0.5 and sd["max_grad_norm"] == 1.5 and sd["skipped_steps"] == 4
    ids_before, tab_before = opt.group_ids.clone(), opt._group_table_full.clone()
    m2, flat2, opt2 = _cpu_optimizer(max_grad_norm=3.0, skip_nonfinite=True)
    ids_ptr, tab_ptr = opt2.group_ids.data_ptr(), opt2._group_table_full.data_ptr()
    opt2.load_state_dict(sd)
    assert opt2.group_ids.data_ptr() == ids_ptr and opt2._group_table_full.data_ptr() == tab_ptr     # in place: graphs stay valid
    assert opt2.state_dict()["param_groups"] == sd["param_groups"]
    assert opt2.max_norm.item() == 1.5 and opt2.stats[3].item() == 4.0
    row = lambda o, n: tuple(o._group_table_full[o.group_ids[o.flat.offsets[n]].item()].tolist())
    assert all(row(opt2, n) == row(opt, n) for n in flat.names)
    # a dictionary written before the new keys existed
    old = {k: v for k, v in sd.items() if k not in ("param_groups", "max_grad_norm", "skipped_steps")}
    m3, flat3, opt3 = _cpu_optimizer(max_grad_norm=3.0, skip_nonfinite=True)
    opt3.load_state_dict(old)
    assert opt3.max_norm.item() == 3.0 and opt3.stats[3].item() == 0.0
    assert opt3.state_dict()["param_groups"]["head.weight"] == (1.0, pytest.approx(0.05))
    # the un-grouped object: keys present and empty; it loads an old dictionary and REFUSES one that carries groups or a
    # clip (resuming a fine-tune with the arguments forgotten would otherwise train with one lr and no clip, silently)
    plain = FlatAdamW(flat3, m3, lr=1e-3, ema_decay=0.99)
    psd = plain.state_dict()
    assert psd["param_groups"] is None and psd["max_grad_norm"] is None and psd["skipped_steps"] == 0
    assert plain.group_ids is None and plain.partials is None and not plain._grouped
    plain.load_state_dict(old)
    plain.load_state_dict(psd)
    with pytest.raises(ValueError, match="built without"):
        plain.load_state_dict(sd)
    assert plain.decay_mask is not None and opt.decay_mask is None          # the decay bytes exist only where they are read
    m4, flat4, opt4 = _cpu_optimizer()                                        # groups, no clip: a state with a clip is refused too
    with pytest.raises(ValueError, match="max_grad_norm"):
        opt4.load_state_dict(sd)
    flat4.close()
    for f in (flat, flat2, flat3):
        f.close()


def test_constructor_errors_and_defaults():
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    m = _Net()
    flat = FlatTrainingState(m)
    ps = dict(m.named_parameters())
    with pytest.raises(ValueError, match="more than one group"):
        FlatAdamW(flat, m, param_groups=[{"params": list(ps.values())}, {"params": [ps["head.bias"]], "lr_scale": 0.5}])
    with pytest.raises(ValueError, match="in no group"):
        FlatAdamW(flat, m, param_groups=[{"params": [p for n, p in ps.items() if n != "head.bias"]}])
    with pytest.raises(ValueError, match="not a trainable parameter"):
        FlatAdamW(flat, m, param_groups=[{"params": list(ps.values()) + [torch.nn.Parameter(torch.zeros(2))]}])
    # names are accepted in place of parameters; missing keys take the constructor's values
    o = FlatAdamW(flat, m, weight_decay=0.1, param_groups=[{"params": [n for n in ps if n != "head.bias"]},
                                                           {"params": ["head.bias"], "weight_decay": 0.0}])
    assert o.group_table.tolist() == [[1.0, pytest.approx(0.1)], [1.0, 0.0]] and o.partials is None and o.stats is None
    with pytest.raises(RuntimeError):
        o.last_stats()
    with pytest.raises(RuntimeError):
        o.set_max_grad_norm(1.0)
    # clipping alone: two groups from weight_decay / no_decay, as the un-grouped object's mask
    o = FlatAdamW(flat, m, weight_decay=0.1, no_decay={"head.bias"}, max_grad_norm=2.0)
    assert o.group_table.tolist() == [[1.0, pytest.approx(0.1)], [1.0, 0.0]]
    off = flat.offsets["head.bias"]
    assert o.group_ids[off:off + 2].tolist() == [1, 1] and int(o.group_ids.sum()) == 2
    assert o.partials.numel() == 1 and o.stats.tolist() == [0.0, 0.0, 0.0, 0.0]
    flat.close()


def test_grad_sumsq_blocks_is_a_pure_host_function():
    from fastvim_amd import _lib
    lib = _lib.lib()
    G = lambda n: lib.fv_grad_sumsq_blocks(ctypes.c_size_t(n))
    assert G(0) == 1 and G(8) == 1 and G(4096) == 1 and G(8192) == 1 and G(8196) == 2
    sizes = [8, 1000, 8192, 8196, 10 ** 5, 7 * 10 ** 6, 28 * 10 ** 6, 10 ** 8, 4 * 10 ** 8, 2 ** 33]
    gs = [G(n) for n in sizes]
    assert gs == sorted(gs) and gs[-1] == 1024 and G(2 ** 40) == 1024                 # non-decreasing, capped
    assert G(7 * 10 ** 6) == -(-(7 * 10 ** 6 // 4) // 2048)                         # two trips of 1024 float4 per workgroup
    assert [G(n) for n in sizes] == gs                                                # a function of n alone
