"""Measure the MAE token bookkeeping on the HIP path (csrc/mae_tokens.hip, ``MaskedAutoencoderViM.fused_tokens``) on the GPU,
in ONE process:

  * step: the graph-replayed MAE-B pre-training step (batch 128, bf16, built as tools/bench_mae_lh.py::make_step builds it)
    with ``fused_tokens`` off and on, rounds alternating between the two; the same for ``mae_FastVim_huge_dec512d2b`` at the
    largest batch of tools/bench_mae_lh.py's list at which BOTH variants fit (``--no-huge`` skips it and says so);
  * kernels: the plan launch, the masking gather and its adjoint, the odd layers' permute, and the decoder assembly forward
    and backward, stand-alone on HBM-cold rotated operands at (128, 196 -> 49, 768) and (128, 256 -> 64, 1280), bf16 tokens,
    next to a plain copy of the same bytes (``floor_ratio`` as in bench.py).

    python tools/bench_mae_tokens.py          # --no-step / --no-huge / --no-kernels skip a part

The per-step kernel traces are taken in a run of their own (the profiler slows the host):

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_mae_tokens.py --trace-step on     # or: off
    python tools/bench_mae_tokens.py --fold DIR/.../*_results.db profiles/mae_tokens_on_step_kernel_stats.csv

``--trace-step`` builds one variant, then replays ``--steps`` steps between two sentinel launches (``erfinv`` on one element:
a kernel the step does not contain); ``--fold`` keeps the dispatches between the sentinels and divides by the step count.

Every GPU phase runs under its own time limit (a watchdog ends the process when a phase overruns: nothing else is then
started on the device).  The log goes to stdout and to ``--log`` (profiles/mae_tokens_bench.log), the last line one JSON
record.  Sets no threshold."""
import argparse
import contextlib
import csv
import faulthandler
import json
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))

KERNEL_SHAPES = ((128, 14, 14, 49, 768), (128, 16, 16, 64, 1280))        # (B, H, W, K, D)
SENTINEL = "erfinv"


@contextlib.contextmanager
def phase(name, seconds, say):
    import torch
    say(f"== {name} (time limit {seconds} s)")
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
        torch.cuda.synchronize()
    finally:
        faulthandler.cancel_dump_traceback_later()


# ------------------------------------------------------------------------------------------------ step
def make_step(factory, img, batch, fused_tokens):
    """tools/bench_mae_lh.py::make_step with the token switch; returns (replay, loss buffer, flat, keep-alive)."""
    import torch
    from fastvim_amd import models_mae
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    torch.manual_seed(1234)
    model = getattr(models_mae, factory)(img_size=img, fused_tokens=fused_tokens).cuda().train()
    x = torch.randn(batch, 3, img, img, generator=torch.Generator().manual_seed(100)).cuda()
    flat = FlatTrainingState(model)
    no_decay = {n for n, p in model.named_parameters()
                if p.ndim <= 1 or n.endswith(".bias") or n in model.no_weight_decay() or getattr(p, "_no_weight_decay", False)}
    opt = FlatAdamW(flat, model, lr=1.5e-4 * batch / 256, betas=(0.9, 0.95), weight_decay=0.05, no_decay=no_decay, ema_decay=0.9999)
    torch.manual_seed(5678)
    seed = torch.ones((), device="cuda", dtype=torch.float32)

    def fwd_bwd():
        flat.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = model(x, mask_ratio=0.75)[0]
        loss.backward(gradient=seed)
        flat.finish_backward()
        return loss.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fwd_bwd()
            opt.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_buf = fwd_bwd()
        opt.step()
    # a captured graph holds ADDRESSES: everything it touches outside its private pool must outlive it
    return graph.replay, loss_buf, flat, (graph, model, opt, x, seed, fwd_bwd)


def timed(fn, steps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def step_pair(name, factory, img, batch, rounds, steps, say):
    """Both variants built, then ``rounds`` alternating rounds of ``steps`` replays -> record."""
    variants = (("fused_tokens off", False), ("fused_tokens on", True))
    built = {}
    with phase(f"{name} step, batch {batch}, bf16, graph replay: build + capture x 2", 900, say):
        for vn, ft in variants:
            built[vn] = make_step(factory, img, batch, ft)
            for _ in range(2):
                built[vn][0]()
    ts = {vn: [] for vn, _ in variants}
    with phase(f"{name} step: {rounds} alternating rounds of {steps} replays", 600, say):
        for _ in range(rounds):
            for vn, _ in variants:
                ts[vn].append(timed(built[vn][0], steps))
    rec = {"batch": batch}
    for vn, _ in variants:
        med = statistics.median(ts[vn])
        say(f"    {vn:<18} median {med:.3f} ms (min {min(ts[vn]):.3f}, max {max(ts[vn]):.3f}) = {batch / med * 1e3:.0f} img/s; "
            f"loss {built[vn][1].item():.6f}")
        rec[vn] = {"ms_per_step": round(med, 3), "ms_rounds": [round(t, 3) for t in ts[vn]], "loss": built[vn][1].item()}
    off, on = ts["fused_tokens off"], ts["fused_tokens on"]
    d = statistics.median(off) - statistics.median(on)
    spread = max(max(off) - min(off), max(on) - min(on))
    say(f"    off - on = {d:+.3f} ms; largest spread of a variant's rounds {spread:.3f} ms: "
        f"{'beyond' if abs(d) > spread else 'within'} the spread")
    rec["off_minus_on_ms"] = round(d, 3)
    rec["rounds_spread_ms"] = round(spread, 3)
    for vn, _ in variants:
        built[vn][2].close()
    return rec


# ------------------------------------------------------------------------------------------------ kernels
def kernel_rows(B, H, W, K, D, curve, say):
    import torch
    from bench import floor_us, rotating, time_kernel
    from fastvim_amd import _lib as L
    from fastvim_amd import mae_tokens as MT
    Ln = H * W
    g = torch.Generator().manual_seed(0)
    noise = torch.rand(B, Ln, generator=g).cuda()
    plan = MT.mask_plan(noise, (H, W), K)
    bf = torch.bfloat16
    T = {"full": torch.randn(B, Ln, D, generator=g).to(bf).cuda(), "kept": torch.randn(B, K, D, generator=g).to(bf).cuda(),
         "dout": torch.randn(B, Ln, D, generator=g).cuda(), "noise": noise}
    mt = torch.randn(1, 1, D, generator=g).cuda()
    pos = torch.randn(1, Ln, D, generator=g).cuda()
    nblocks = -(-(B * Ln) // MT.DECODER_ROWS_PER_BLOCK)
    partials = torch.empty(nblocks, D, device="cuda", dtype=torch.float64)
    dmt = torch.empty(D, device="cuda")
    dx = torch.empty(B, K, D, device="cuda", dtype=bf)
    lib, i32, p_ = L.lib(), L.i32, L.ptr

    def dec_bwd(s):
        rc = lib.fv_mae_decoder_tokens_bwd(p_(s["dout"]), p_(plan.restore_index), p_(dx), i32(L.FV_BF16), p_(partials), i32(nblocks),
                                           p_(dmt), i32(B), i32(Ln), i32(K), i32(D), L.stream_of(dx))
        L.check(rc, "mae_decoder_tokens_bwd")

    kept_b, full_b = B * K * D * 2, B * Ln * D * 2
    rows = (
        ("plan (one launch)", lambda s: MT.mask_plan(s["noise"], (H, W), K), ("noise",), None),
        ("masking gather L -> K", lambda s: MT._gather(s["full"], plan.keep_index, bf), ("full",), 2 * kept_b),
        ("its adjoint K -> L", lambda s: MT._gather(s["kept"], plan.restore_index, bf), ("kept",), kept_b + full_b),
        ("odd-layer permute K -> K", lambda s: MT._gather(s["kept"], plan.order_index, bf), ("kept",), 2 * kept_b),
        ("decoder tokens fwd", lambda s: MT._DecoderTokensFn.apply(s["kept"], mt, pos, plan.restore_index), ("kept",),
         kept_b + Ln * D * 4 + B * Ln * D * 4),
        ("decoder tokens bwd (2 launches)", dec_bwd, ("dout",), B * Ln * D * 4 + kept_b + nblocks * D * 16),
    )
    res = {}
    for rep in (1, 2):
        for name, fn, names, nbytes in rows:
            us = time_kernel(rotating(fn, T, names, nbytes or 1 << 20)) * 1e6
            rec = {"us": round(us, 2)}
            if nbytes:
                fl = floor_us(curve, nbytes / 1e6)
                rec.update({"MB": round(nbytes / 1e6, 2), "floor_us": round(fl, 2), "floor_ratio": round(us / fl, 2),
                            "TBps": round(nbytes / us / 1e6, 3)})
                say(f"    [{rep}] {name:<32} {us:8.1f} us  {nbytes / 1e6:7.1f} MB  {rec['TBps']:.2f} TB/s  copy {fl:7.1f} us  "
                    f"floor_ratio {rec['floor_ratio']:.2f}")
            else:
                say(f"    [{rep}] {name:<32} {us:8.1f} us")
            res[f"{name} #{rep}"] = rec
    return res


# ------------------------------------------------------------------------------------------------ traces
def trace_step(variant, batch, steps):
    import torch
    replay, loss_buf, flat, keep = make_step("mae_FastVim_base_dec512d2b", 224, batch, variant == "on")
    one = torch.full((1,), 0.5, device="cuda")
    torch.manual_seed(777)          # the in-graph torch.rand of both variants' runs then draws the same masking noise
    for _ in range(2):
        replay()
    torch.cuda.synchronize()
    first = loss_buf.item()
    torch.erfinv(one)
    for _ in range(steps):
        replay()
    torch.erfinv(one)
    torch.cuda.synchronize()
    print(f"traced {steps} replayed steps, fused_tokens {variant}: loss after 2 replays {first.hex()}, after {2 + steps} "
          f"{loss_buf.item().hex()}", flush=True)
    flat.close()


def fold(db_path, out_path, steps):
    import sqlite3
    from rocpd_stats import short
    db = sqlite3.connect(db_path)
    marks = [r[0] for r in db.execute("select start from kernels where name like ? order by start", (f"%{SENTINEL}%",))]
    if len(marks) != 2:
        raise SystemExit(f"expected 2 sentinel dispatches, found {len(marks)}")
    rows = db.execute("select name, count(*), sum(end - start), avg(end - start), min(end - start), max(end - start) from kernels "
                      "where start > ? and start < ? group by name order by 3 desc", (marks[0], marks[1])).fetchall()
    total = sum(r[2] for r in rows) or 1
    calls = sum(r[1] for r in rows)
    with open(out_path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Name", "CallsPerStep", "TotalNsPerStep", "AverageNs", "MinNs", "MaxNs", "Percentage"])
        for n, c, t, a, mn, mx in rows:
            w.writerow([short(n), round(c / steps, 2), round(t / steps), round(a, 1), mn, mx, round(100.0 * t / total, 3)])
    print(f"{len(rows)} kernels, {calls / steps:.1f} dispatches and {total / steps / 1e6:.3f} ms of kernel time per step -> {out_path}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10, help="replayed steps per timed round / in the traced window")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-huge", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--trace-step", choices=["off", "on"], help="only: build one variant and replay --steps steps between sentinels")
    ap.add_argument("--fold", nargs=2, metavar=("DB", "CSV"), help="only: fold a rocprofv3 results.db of --trace-step into a CSV")
    ap.add_argument("--log", default=os.path.join(R, "profiles", "mae_tokens_bench.log"))
    args = ap.parse_args()
    if args.fold:
        return fold(args.fold[0], args.fold[1], args.steps)
    import torch
    import fastvim_amd  # noqa: F401  (sets the graph-capture switch before HIP initialises)
    if not torch.cuda.is_available():
        raise SystemExit("bench_mae_tokens.py needs a GPU")
    if args.trace_step:
        faulthandler.dump_traceback_later(900, exit=True)
        return trace_step(args.trace_step, args.batch, args.steps)
    lines, out = [], {}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush_log():
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")

    say(f"{torch.cuda.get_device_name()}: MAE token bookkeeping, fused_tokens off / on")
    if not args.no_step:
        out["step MAE-B 224"] = step_pair("MAE-B", "mae_FastVim_base_dec512d2b", 224, args.batch, args.rounds, args.steps, say)
        torch.cuda.empty_cache()
        flush_log()
        if args.no_huge:
            say("== MAE-H step: not run (--no-huge)")
            out["step MAE-H 224"] = "not run"
        else:
            import bench_mae_lh as LH
            _, d, depth, img, patch = LH.CONFIGS["MH224"]
            free = torch.cuda.mem_get_info()[0]
            batch = LH.pick_batch(d, depth, img, patch, free // 2)           # two variants live at once
            if batch is None:
                say(f"== MAE-H step: not run (no batch of {LH.BATCHES} fits twice into {free / 2**30:.1f} GB)")
                out["step MAE-H 224"] = "not run"
            else:
                out["step MAE-H 224"] = step_pair("MAE-H", "mae_FastVim_huge_dec512d2b", 224, batch, args.rounds, args.steps, say)
            torch.cuda.empty_cache()
        flush_log()
    if not args.no_kernels:
        from bench import floor_curve
        with phase("copy floor", 240, say):
            curve = floor_curve(torch.bfloat16, sizes_mb=(8, 16, 32, 64, 112, 160))
            say("  copy floor (MB moved, us): " + ", ".join(f"({a:.0f}, {b:.1f})" for a, b in curve))
            out["floor_curve"] = [(round(a, 1), round(b, 2)) for a, b in curve]
        out["kernels"] = {}
        for B, H, W, K, D in KERNEL_SHAPES:
            with phase(f"kernels at ({B}, {H * W} -> {K}, {D}), bf16 tokens, HBM-cold", 300, say):
                out["kernels"][f"({B}, {H * W} -> {K}, {D})"] = kernel_rows(B, H, W, K, D, curve, say)
            torch.cuda.empty_cache()
            flush_log()
    lines.append(json.dumps(out))
    print(lines[-1])
    flush_log()


if __name__ == "__main__":
    main()
