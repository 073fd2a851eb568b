"""The validation step, the parts that need no GPU: the C ABI of csrc/eval.hip, the argument checks, the host reduction
from counts to metrics (fastvim_amd.evaluate.metrics_from_counts) and the merge of two ranks' blocks over gloo."""
import ctypes
import math
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import eval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("fv_swap_params_ema", "fv_eval_accumulate")


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
    from fastvim_amd import evaluate
    assert int(re.search(r"#define\s+FV_EVAL_ACC_HEAD\s+(\d+)", hdr).group(1)) == evaluate.ACC_HEAD
    assert evaluate.block_words(1000) == 2003


def test_argument_checks_need_no_gpu():
    """Null pointers, an unsupported dtype and too many classes are refused through fv_last_error before any launch."""
    from fastvim_amd import _lib
    lib = _lib.lib()
    i, p, z = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    a, b, c = p(64), p(128), p(256)              # non-null, aligned: refused calls never dereference them
    for args in ((p(0), b, c), (a, p(0), c), (a, b, p(0))):
        assert lib.fv_swap_params_ema(*args, i(1), z(8), p(0)) == -1
        assert b"null pointer" in lib.fv_last_error()
    assert lib.fv_swap_params_ema(a, b, c, i(7), z(8), p(0)) == -1
    assert b"fp32, bf16 or fp16" in lib.fv_last_error()
    assert lib.fv_swap_params_ema(p(66), b, c, i(1), z(8), p(0)) == -1
    assert b"aligned" in lib.fv_last_error()
    assert lib.fv_swap_params_ema(a, a, c, i(1), z(8), p(0)) == -1
    assert b"same buffer" in lib.fv_last_error()
    assert lib.fv_swap_params_ema(a, b, c, i(1), z(0), p(0)) == 0          # nothing to do, nothing launched

    def acc(logits=a, dtype=0, labels=a, nv=a, rows=a, corr=a, blk=a, B=4, C=10):
        return lib.fv_eval_accumulate(logits, i(dtype), labels, nv, rows, corr, blk, i(B), i(C), p(0))
    for kw in ("logits", "labels", "nv", "rows", "corr", "blk"):
        assert acc(**{kw: p(0)}) == -1
        assert b"null pointer" in lib.fv_last_error()
    assert acc(dtype=2) == -1
    assert b"fp32 or bf16" in lib.fv_last_error()
    assert acc(C=2049) == -1
    assert b"2048" in lib.fv_last_error()
    assert acc(B=0) == -1 and acc(C=0) == -1
    assert acc(blk=p(68)) == -1
    assert b"8-byte" in lib.fv_last_error()


def test_python_argument_checks():
    from fastvim_amd.evaluate import EvalMetrics, metrics_from_counts
    with pytest.raises(ValueError, match="2048"):
        EvalMetrics(4096, "cpu")
    m = EvalMetrics(10, "cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        m.update(torch.zeros(4, 10), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="n_valid"):
        m.update(torch.zeros(4, 10), torch.zeros(4, dtype=torch.int64), n_valid=5)
    with pytest.raises(ValueError, match="block"):
        metrics_from_counts(torch.zeros(7, dtype=torch.int64), 10)


def test_metrics_from_hand_made_counts():
    """4 classes, class 2 never seen, one sample with an out-of-range label (in n, in no class):
    support [3, 2, 0, 4], hit [3, 1, 0, 1]: micro = 5 / 10, macro = (1 + 1/2 + 1/4) / 3 over the three classes present."""
    from fastvim_amd.evaluate import metrics_from_counts
    blk = R.pack_block(12.5, 10, 5, [3, 2, 0, 4], [3, 1, 0, 1])
    m = metrics_from_counts(blk, 4)
    assert m["n"] == 10 and m["loss"] == 1.25 and m["acc_micro"] == 0.5
    assert m["acc_macro"] == pytest.approx((1.0 + 0.5 + 0.25) / 3, rel=1e-15)
    assert m["support"].tolist() == [3, 2, 0, 4] and m["hit"].tolist() == [3, 1, 0, 1]
    assert m["support"].dtype == torch.int64
    # counts beyond 2**31 and a loss sum that fp32 could not hold exactly
    big = R.pack_block(2.0 ** 40 + 0.5, 2 ** 40, 2 ** 39, [2 ** 39, 2 ** 39], [2 ** 38, 2 ** 38])
    m = metrics_from_counts(big, 2)
    assert m["n"] == 2 ** 40 and m["acc_micro"] == 0.5 and m["acc_macro"] == 0.5 and m["loss"] == (2.0 ** 40 + 0.5) / 2 ** 40


def test_metrics_of_an_empty_block_are_nan():
    """n = 0: the mean of no samples is NaN (torch.empty(0).mean()), nothing raises; counts are zeros."""
    from fastvim_amd.evaluate import block_words, metrics_from_counts
    m = metrics_from_counts(torch.zeros(block_words(3), dtype=torch.int64), 3)
    assert m["n"] == 0 and math.isnan(m["loss"]) and math.isnan(m["acc_micro"]) and math.isnan(m["acc_macro"])
    assert m["support"].tolist() == [0, 0, 0] and m["hit"].tolist() == [0, 0, 0]
    # samples seen, all with out-of-range labels: micro is defined, macro has no class to average over
    m = metrics_from_counts(R.pack_block(0.0, 4, 0, [0, 0, 0], [0, 0, 0]), 3)
    assert m["acc_micro"] == 0.0 and m["loss"] == 0.0 and math.isnan(m["acc_macro"])


def test_reference_agrees_with_torch_cross_entropy():
    """The fp64 reference the GPU tests compare against, itself against torch's own loss on the valid rows."""
    x, y = R.make_batch(9, 10, torch.float32, 7, seed=3)
    ref = R.reference(x, y, 7, 10)
    want = torch.nn.functional.cross_entropy(x[:7].double(), y[:7], reduction="sum")
    assert abs(ref["loss_sum"] - want.item()) <= 1e-12 * abs(want.item())
    assert ref["n"] == 7 and ref["n_correct"] == int((x[:7].argmax(1) == y[:7]).sum())
    assert int(ref["support"].sum()) == 7 and torch.equal(ref["support"], torch.bincount(y[:7], minlength=10))
    assert bool((y[7:] == -1).all()) and bool((x[7:].abs() > 1e38).all()) and bool(torch.isfinite(x).all())
    # a label outside [0, C): seen, loss 0, never correct, in no class
    y2 = y.clone()
    y2[0] = 10
    r2 = R.reference(x, y2, 7, 10)
    assert r2["n"] == 7 and int(r2["support"].sum()) == 6 and r2["loss_rows"][0] == 0.0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_block(rank):
    if rank == 0:
        return R.pack_block(10.25, 7, 4, [3, 0, 4, 0], [2, 0, 2, 0])
    return R.pack_block(3.5, 5, 1, [1, 2, 2, 0], [0, 1, 0, 0])


def _merge_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from fastvim_amd.evaluate import allreduce_blocks, metrics_from_counts
    mine = _rank_block(rank)
    keep = mine.clone()
    a, b = allreduce_blocks([mine, mine], None)              # two blocks, one all-reduce (the live and the EMA block)
    assert torch.equal(mine, keep) and torch.equal(a, b) and a.dtype == torch.int64
    torch.save({"block": a, "metrics": metrics_from_counts(a, 4)}, out + f".{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_merge_to_the_single_process_result(tmp_path):
    from fastvim_amd.evaluate import allreduce_blocks, metrics_from_counts
    out = str(tmp_path / "merged.pt")
    mp.spawn(_merge_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    whole = R.pack_block(13.75, 12, 5, [4, 2, 6, 0], [2, 1, 2, 0])          # the counts of both ranks' samples together
    want = metrics_from_counts(whole, 4)
    for rank in range(2):
        got = torch.load(out + f".{rank}", weights_only=False)
        assert torch.equal(got["block"], whole)
        for k in ("loss", "acc_micro", "acc_macro", "n"):
            assert got["metrics"][k] == want[k], k
        assert torch.equal(got["metrics"]["support"], want["support"]) and torch.equal(got["metrics"]["hit"], want["hit"])
    assert want["n"] == 12 and want["acc_micro"] == 5 / 12 and want["acc_macro"] == pytest.approx((0.5 + 0.5 + 1 / 3) / 3, rel=1e-15)
    # without a process group the function is the identity (on copies)
    (same,) = allreduce_blocks([whole], None)
    assert torch.equal(same, whole) and same.data_ptr() != whole.data_ptr()
