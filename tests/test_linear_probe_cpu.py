"""Linear probing, the parts that need no GPU: the probe head against what the reference's ``SupervisedModule.__init__``
leaves on a model (tests/golden/linear_probe.pt), the optimizer's host-side tables, the C ABI, and the all-gather of the
BatchNorm statistics table over gloo."""
import ctypes
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("fv_bn1d_stats", "fv_bn1d_apply", "fv_bn1d_bwd", "fv_sgd_flat", "fv_lars_partials_per_segment",
               "fv_lars_sumsq_partials", "fv_lars_flat")


def _probe_model(gold):
    from fastvim_amd.fastvim import VisionMamba
    from fastvim_amd.linear_probe import attach_probe_head
    torch.manual_seed(0)
    return attach_probe_head(VisionMamba(**gold["probe"]["model_kwargs"]))


def test_attach_probe_head_matches_the_reference_module(golden):
    gold = golden("linear_probe.pt")
    from fastvim_amd.linear_probe import ProbeBatchNorm1d
    m = _probe_model(gold)
    assert [(n, bool(p.requires_grad)) for n, p in m.named_parameters()] == [tuple(f) for f in gold["probe"]["flags"]]
    assert sorted(k for k in m.state_dict() if k.startswith("head.")) == gold["probe"]["head_keys"] == [
        "head.0.num_batches_tracked", "head.0.running_mean", "head.0.running_var", "head.1.bias", "head.1.weight"]
    bn = m.head[0]
    assert isinstance(bn, ProbeBatchNorm1d) and isinstance(bn, torch.nn.BatchNorm1d)
    assert (bn.eps, bn.momentum, bn.affine) == (gold["probe"]["bn"]["eps"], gold["probe"]["bn"]["momentum"], gold["probe"]["bn"]["affine"])
    assert bn.eps == 1e-6 and bn.num_features == m.head[1].in_features
    # a reference probe checkpoint loads by key
    sd = {k: torch.randn_like(v) if v.is_floating_point() else torch.tensor(7) for k, v in m.state_dict().items()}
    m.load_state_dict(sd, strict=True)
    assert int(m.head[0].num_batches_tracked) == 7 and torch.equal(m.head[0].running_var, sd["head.0.running_var"])


def test_probe_head_weight_is_redrawn_with_std_001(golden):
    """64 000 draws of N(0, 0.01) cut at +-2 (200 sigma: no cut): the sample std is 0.01 +- 0.01 / sqrt(2 * 64000) = 2.8e-5;
    7 sigma allowed.  The recorded reference draw lies in the same band."""
    gold = golden("linear_probe.pt")
    m = _probe_model(gold)
    w = m.head[1].weight.detach()
    assert w.numel() == 64000
    assert abs(w.std().item() - 0.01) < 2e-4 and abs(gold["probe"]["head_weight_std"] - 0.01) < 2e-4
    assert abs(w.mean().item()) < 2e-4


def test_probe_batchnorm_raises_on_cpu():
    from fastvim_amd.linear_probe import ProbeBatchNorm1d
    bn = ProbeBatchNorm1d(8, affine=False, eps=1e-6)
    assert sorted(bn.state_dict()) == sorted(torch.nn.BatchNorm1d(8, affine=False).state_dict())
    with pytest.raises(RuntimeError, match="GPU only"):
        bn(torch.randn(4, 8))


def test_flat_sgd_tables_on_a_cpu_model(golden):
    """The flat state over a probe model holds the head only; FlatSGD's decay bytes follow ``no_decay``, the LARS segment
    table has one row per parameter with ``ndim > 1`` marking the weight."""
    gold = golden("linear_probe.pt")
    from fastvim_amd.flat import FlatSGD, FlatTrainingState, build_segment_table
    m = _probe_model(gold)
    frozen_before = {n: p.detach().clone() for n, p in m.named_parameters() if not p.requires_grad}
    with FlatTrainingState(m) as flat:
        assert flat.names == ["head.1.weight", "head.1.bias"]
        nw, nb = 1000 * 64, 1000
        assert flat.offsets == {"head.1.weight": 0, "head.1.bias": nw} and flat.param_flat.numel() == nw + nb
        opt = FlatSGD(flat, m, lr=0.1, momentum=0.9, weight_decay=0.05, no_decay=("head.1.bias",))
        assert opt.segments is None and opt.momentum_buf.numel() == nw + nb and float(opt.lr) == pytest.approx(0.1)
        assert opt.decay_mask.dtype == torch.uint8
        assert bool(opt.decay_mask[:nw].all()) and not bool(opt.decay_mask[nw:].any())
        opt.set_lr(0.25)
        assert float(opt.lr) == 0.25
        lars = FlatSGD(flat, m, lr=0.1, lars=True, weight_decay=0.05)
        assert lars.segments.dtype == torch.int64 and lars.segments.tolist() == [[0, nw, 1], [nw, nb, 0]]
        assert lars.partials.numel() == 2 * 2 * 64 and lars.norms.shape == (2, 3)
        sd = lars.state_dict()
        assert sorted(sd["state"]) == ["head.1.bias", "head.1.weight"] and sd["lars"] is True
        assert sd["state"]["head.1.weight"]["momentum_buffer"].shape == (1000, 64)
        sd["state"]["head.1.bias"]["momentum_buffer"].fill_(3.0)
        lars.load_state_dict(sd)
        assert bool((lars.momentum_buf[nw:] == 3.0).all()) and not bool(lars.momentum_buf[:nw].any())
        with pytest.raises(ValueError, match="lars"):
            opt.load_state_dict(sd)
    # frozen parameters are not part of the flat state and keep their own storage
    for n, p in m.named_parameters():
        if not p.requires_grad:
            assert torch.equal(p, frozen_before[n]) and p.grad is None and getattr(p, "_fv_shadow", None) is None
    # padding between parameters: offsets are multiples of 8 elements, lengths are the true element counts
    t = build_segment_table(["w", "b", "s"], {"w": 0, "b": 240, "s": 256}, {"w": (10, 24), "b": (10,), "s": ()})
    assert t.tolist() == [[0, 240, 1], [240, 10, 0], [256, 1, 0]]


def test_freeze_shadows_on_a_cpu_model(golden):
    gold = golden("linear_probe.pt")
    from fastvim_amd.linear_probe import freeze_shadows
    from fastvim_amd.mamba_simple_faster import _shadow
    m = _probe_model(gold)
    buf = freeze_shadows(m)
    assert buf.dtype == torch.bfloat16 and buf.numel() % 8 == 0
    w = m.layers[0].mixer.in_proj.weight
    sh = _shadow(w, torch.bfloat16)
    assert sh.data_ptr() == w._fv_shadow.data_ptr() and torch.equal(sh, w.detach().to(torch.bfloat16))
    assert getattr(m.head[1].weight, "_fv_shadow", None) is None            # trainable: left to the flat training state
    with torch.no_grad():
        w.mul_(2.0)                                                          # an in-place write (load_state_dict) ...
    assert torch.equal(_shadow(w, torch.bfloat16), w.detach().to(torch.bfloat16))      # ... is re-cast by the version check
    assert _shadow(w, torch.bfloat16).data_ptr() == sh.data_ptr()


def test_new_symbols_are_declared_and_the_abi_version_stays():
    from fastvim_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fastvim_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fv_[a-z0-9_]+)\s*\(", hdr))
    import fastvim_amd.build as fb
    fb.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib.C_ABI_SYMBOLS and hasattr(lib, s), s
    assert int(re.search(r"#define\s+FV_ABI_VERSION\s+(\d+)", hdr).group(1)) == 3 == lib.fv_version()
    assert lib.fv_lars_partials_per_segment() == 64


def test_argument_checks_need_no_gpu():
    """Invalid arguments are refused through fv_last_error before anything touches the device."""
    from fastvim_amd import _lib
    lib = _lib.lib()
    i, p, f, z = ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_size_t
    assert lib.fv_bn1d_stats(p(0), i(0), p(0), i(4), i(8), p(0)) == -1
    assert b"null pointer" in lib.fv_last_error()
    assert lib.fv_bn1d_stats(p(16), i(2), p(16), i(4), i(8), p(0)) == -1
    assert b"fp32 or bf16" in lib.fv_last_error()
    assert lib.fv_bn1d_apply(p(16), i(0), p(0), i(0), p(0), p(0), p(0), p(16), p(16), p(16), i(4), i(8), f(1e-6), f(0.1), i(1), p(0)) == -1
    assert b"table" in lib.fv_last_error()
    assert lib.fv_bn1d_apply(p(16), i(0), p(0), i(0), p(0), p(0), p(0), p(16), p(16), p(16), i(4), i(8), f(1e-6), f(0.1), i(0), p(0)) == -1
    assert b"running statistics" in lib.fv_last_error()
    assert lib.fv_sgd_flat(p(16), p(16), p(16), p(0), p(16), p(16), f(0.9), f(0.0), f(1.0), z(6), p(0)) == -1
    assert b"multiple of 4" in lib.fv_last_error()
    assert lib.fv_lars_flat(p(16), p(16), p(16), p(0), p(16), i(0), p(16), p(16), p(0), f(0.9), f(0.0), f(1e-3), f(1.0), z(8), p(0)) == -1
    assert b"segments" in lib.fv_last_error()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _gather_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from fastvim_amd.linear_probe import gather_table
    d = 5
    row = torch.arange(2 * d + 1, dtype=torch.float32) + 100.0 * rank          # rank r's row: 100 r + [0 .. 2 d]
    row[-1] = 20.0 - 3.0 * rank                                                 # unequal counts
    table = torch.full((world, 2 * d + 1), -1.0)
    got = gather_table(row, table)
    assert got.data_ptr() == table.data_ptr()
    torch.save(table, out + f".{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_statistics_table_all_gather_over_gloo(tmp_path):
    out = str(tmp_path / "table.pt")
    mp.spawn(_gather_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    t0, t1 = torch.load(out + ".0"), torch.load(out + ".1")
    want = torch.stack([torch.arange(11, dtype=torch.float32), torch.arange(11, dtype=torch.float32) + 100.0])
    want[0, -1], want[1, -1] = 20.0, 17.0
    assert torch.equal(t0, want) and torch.equal(t1, want)       # both ranks: the same two rows, in rank order
