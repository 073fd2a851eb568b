"""Time the validation step (fastvim_amd/evaluate.py) on the GPU, in ONE process:

  * the graph-replayed ``ValidationStep`` at FastVim-T 224 px, batch 128, bf16 -- the batch under the live and the EMA
    weights -- against TWO graph-replayed ``no_grad`` evaluation forwards of the same model and batch, alternated in the
    same run.  The difference is what the feature adds: two swaps, two ``refresh_transposed`` and the metric launches;
  * ``fv_swap_params_ema`` stand-alone, HBM-cold (operand sets rotated past the Infinity Cache, bench.py's ``rotating``),
    at FastVim-T size (7.17 M elements) and FastVim-B size (97.7 M), against a plain copy kernel moving the same bytes
    (18 B per element) in the same run: the ``floor_ratio`` of bench.py (1.0 = the launch costs what moving its bytes costs);
  * ``fv_eval_accumulate`` at (128, 1000) bf16 logits.

    python tools/bench_eval.py            # --no-model times the kernels only; --sizes 7.17 picks swap sizes (M elements)

Reads nothing outside the repository and sets no threshold.  The log goes to stdout and to ``--log``
(profiles/eval_bench.log), the last line one JSON record.  Give it a time limit of its own when it runs next to other
work (``timeout -k 10 600 python tools/bench_eval.py``)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import torch  # noqa: E402
import fastvim_amd  # noqa: E402,F401  (sets the graph-capture switch before HIP initialises)
from bench import rotating, time_kernel  # noqa: E402

CLASSES, IMG, BATCH = 1000, 224, 128


def alternating(runs, iters, rounds):
    """{name: (median, min, max) ms per call}: every round times each candidate once, ``iters`` calls between two events."""
    for run in runs.values():
        run()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for k, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                run()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / iters)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def bench_model(steps, rounds, say):
    from fastvim_amd import fastvim as fv
    from fastvim_amd.evaluate import ValidationStep
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    from fastvim_amd.losses import CrossEntropyLoss
    torch.manual_seed(1234)
    model = fv.vim_tiny_patch16_224_final_pool_mean_abs_pos_embed_with_noclstok_div2(img_size=IMG, num_classes=CLASSES).cuda().train()
    gen = torch.Generator().manual_seed(100)
    x = torch.randn(BATCH, 3, IMG, IMG, generator=gen).cuda()
    labels = torch.randint(0, CLASSES, (BATCH,), generator=gen).cuda()
    flat = FlatTrainingState(model)
    opt = FlatAdamW(flat, model, lr=1e-3, weight_decay=0.05, ema_decay=0.9998)
    crit = CrossEntropyLoss()
    for _ in range(2):                           # two training steps: the EMA weights differ from the live ones
        flat.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = crit(model(x), labels)
        loss.backward()
        opt.step()
    val = ValidationStep(model, flat, opt, x, labels)
    live_only = ValidationStep(model, flat, opt, x, labels, ema=False)

    def two_forwards():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return model(x), model(x)
    model.eval()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        two_forwards()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, pool=torch.cuda.graph_pool_handle()):
        keep = two_forwards()
    model.train()
    res = alternating({"validation_step": val.step, "two_forwards": g.replay, "validation_step_live_only": live_only.step},
                      steps, rounds)
    torch.cuda.synchronize()
    out = val.compute()
    del keep
    flat.close()
    rec = {"batch": BATCH, "graph_replayed": val.graph is not None, "elements": flat.param_flat.numel(),
           **{k + "_ms": [round(t, 4) for t in v] for k, v in res.items()}}
    rec["overhead_ms"] = round(res["validation_step"][0] - res["two_forwards"][0], 4)
    rec["img_per_s"] = round(BATCH / res["validation_step"][0] * 1e3, 1)
    say(f"FastVim-T {IMG} px, batch {BATCH}, bf16, {flat.param_flat.numel() / 1e6:.2f} M flat elements "
        f"(median [min .. max] ms over {rounds} rounds of {steps}):")
    for k, (m, lo, hi) in res.items():
        say(f"  {k:28s} {m:9.3f}  [{lo:.3f} .. {hi:.3f}]")
    say(f"  overhead (validation step - two forwards) {rec['overhead_ms']:.3f} ms; {rec['img_per_s']} img/s through both weight "
        f"sets; val_loss {out['val_loss']:.4f} val_loss_ema {out['val_loss_ema']:.4f} n {out['n']}")
    return rec


def bench_swap(n, say):
    """One swap launch over ``n`` elements with a bf16 shadow, HBM-cold, against a copy of the same 18 n bytes."""
    from fastvim_amd import _lib as L
    nbytes = 18 * n
    base = {"p": torch.randn(n, device="cuda"), "e": torch.randn(n, device="cuda"),
            "s": torch.zeros(n, device="cuda", dtype=torch.bfloat16)}

    def swap(t):
        rc = L.lib().fv_swap_params_ema(L.ptr(t["p"]), L.ptr(t["e"]), L.ptr(t["s"]), L.i32(L.FV_BF16), ctypes.c_size_t(n),
                                        L.stream_of(t["p"]))
        L.check(rc, "swap_params_ema")
    fns = rotating(swap, base, ("p", "e", "s"), nbytes, cap=8)
    us = time_kernel(fns) * 1e6
    sets = len(fns)
    del fns, base
    half = nbytes // 8                            # fp32 elements of the copy's source: half the bytes read, half written
    cbase = {"a": torch.randn(half, device="cuda"), "b": torch.empty(half, device="cuda")}
    cf = rotating(lambda t: t["b"].copy_(t["a"]), cbase, ("a", "b"), nbytes, cap=8)
    fl = time_kernel(cf) * 1e6
    del cf, cbase
    torch.cuda.empty_cache()
    rec = {"elements": n, "MB": round(nbytes / 1e6, 1), "us": round(us, 2), "copy_us": round(fl, 2), "floor_ratio": round(us / fl, 3),
           "TBps": round(nbytes / us / 1e6, 3), "copy_TBps": round(nbytes / fl / 1e6, 3), "operand_sets": sets}
    say(f"  fv_swap_params_ema {n / 1e6:7.2f} M elements ({rec['MB']:7.1f} MB): {us:9.1f} us = {rec['TBps']:.2f} TB/s; copy of the "
        f"same bytes {fl:9.1f} us = {rec['copy_TBps']:.2f} TB/s; floor_ratio {rec['floor_ratio']:.2f}  [{sets} operand sets]")
    return rec


def bench_accumulate(say):
    from fastvim_amd.evaluate import EvalMetrics
    x = torch.randn(BATCH, CLASSES, device="cuda").to(torch.bfloat16)
    y = torch.randint(0, CLASSES, (BATCH,), device="cuda")
    m = EvalMetrics(CLASSES, "cuda")
    m.update(x, y)
    us = time_kernel(lambda: m.accumulate(x, y, m._nv), iters=50) * 1e6
    say(f"  fv_eval_accumulate ({BATCH}, {CLASSES}) bf16, two launches, cache-warm: {us:.1f} us")
    return {"us": round(us, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="7.17,97.7", help="swap sizes in M elements")
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--log", default=os.path.join(R, "profiles", "eval_bench.log"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    assert torch.cuda.is_available(), "bench_eval.py needs a GPU"
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    rec = {}
    if not a.no_model:
        rec["model"] = bench_model(a.steps, a.rounds, say)
    say("kernels (device time per launch from a replayed graph of back-to-back launches):")
    rec["swap"] = []
    for mel in [float(v) for v in a.sizes.split(",") if v]:
        n = int(mel * 1e6) // 8 * 8
        need = 3 * 36 * n + (1 << 30)
        free = torch.cuda.mem_get_info()[0]
        if need > free:
            say(f"  fv_swap_params_ema {mel} M elements: NOT RUN ({need / 2 ** 30:.1f} GiB needed, {free / 2 ** 30:.1f} GiB free)")
            continue
        rec["swap"].append(bench_swap(n, say))
    rec["accumulate"] = bench_accumulate(say)
    say(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    with open(a.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
