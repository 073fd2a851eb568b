"""Time the graph-replayed fine-tuning step of the large models on the GPU, in ONE process:

    FastVim-L  224 px  (d_model 1024, depth 48, patch 16: 14 x 14 grid)
    FastVim-H  224 px  (d_model 1280, depth 64, patch 14: 16 x 16 grid)
    FastVim-H  448 px  (32 x 32 grid)

each in bf16 with the recipe of mae/config/finetune_FastVimL.yaml / finetune_FastVimH.yaml / finetune_FastVimH_448.yaml:
layer-wise lr decay 0.75, max_grad_norm 3.0, Mixup 0.8 / CutMix 1.0 / label smoothing 0.1 inside the step,
scaling_factor 0.25, DropPath.  Per configuration:

  * the largest per-GPU batch of {128, 64, 32, 16, 8} whose ESTIMATED footprint fits the free device memory
    (torch.cuda.mem_get_info) -- decided from the state size before anything is allocated, never by running out;
  * ms per step and images / s (median and spread over --rounds rounds of --steps replayed steps);
  * the per-kernel table of the replayed step (name, calls per step, average us, share), from torch.profiler;
  * the four mixer row kernels whose launch forms d_inner 2048 / 2560 needed (conv + pool forward / adjoint, combine
    forward / adjoint) at the configuration's shape, HBM-cold, against a plain copy kernel moving the same algorithmic
    bytes in the same run: the ``floor_ratio`` of bench.py (1.0 = the launch costs what moving its bytes costs), with the
    launch plan fv_mixer_plan reports for the shape.

    python tools/bench_lh.py                      # all three; --configs L224,H224 picks; --no-step / --no-kernels skip a part

Reads nothing outside the repository.  Sets no threshold: the parent of these kernels cannot run the models, so there is
no number to compare with.  The log goes to stdout and to ``--log`` (profiles/lh_bench.log), the last line one JSON
record.  Give it a time limit of its own when it runs next to other work (``timeout -k 10 900 python tools/bench_lh.py``)."""
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
from bench import floor_curve, floor_us, rotating, time_kernel  # noqa: E402

CLASSES = 1000
BATCHES = (128, 64, 32, 16, 8)
#          name: (factory, d_model, depth, img, patch, drop_path_rate)
CONFIGS = {
    "L224": ("vim_large_patch16_224_final_pool_mean_abs_pos_embed_with_noclstok_div2", 1024, 48, 224, 16, 0.3),
    "H224": ("vim_huge_patch14_224_final_pool_mean_abs_pos_embed_with_noclstok_div2", 1280, 64, 224, 14, 0.3),
    "H448": ("vim_huge_patch14_224_final_pool_mean_abs_pos_embed_with_noclstok_div2", 1280, 64, 448, 14, 0.3),
}


def param_count(d, depth, img, patch):
    d_in, R_, N = 2 * d, -(-d // 16), 16
    mixer = 2 * d_in * d + d * d_in + 2 * d_in + 2 * (d_in * N + d_in + d_in * 5 + (R_ + 2 * N) * d_in + d_in * R_ + d_in)
    tokens = (img // patch) ** 2
    return depth * (mixer + d) + tokens * d + d * 3 * patch * patch + d + CLASSES * d + CLASSES + d


def footprint_bytes(d, depth, img, patch, batch):
    """Estimated device bytes of the replayed step at ``batch``: the flat training state (fp32 parameters, gradients, two
    Adam moments, EMA; bf16 shadow and the transposed projection shadows) and what autograd keeps per layer in bf16
    storage: the block input (fp32 residual + bf16 normalised rows), xz (2 d_inner), skip, gated output, out_proj product;
    the backward's transients (d xz, d_o, d gated) once.  x 1.25 for the graphs' private pool and allocator slack."""
    n = param_count(d, depth, img, patch)
    state = n * (5 * 4 + 2 * 2)
    tok = batch * (img // patch) ** 2
    d_in = 2 * d
    per_layer = tok * (d * (4 + 2 + 2) + 2 * d_in * 2 + 2 * d_in * 2)
    transient = tok * (2 * d_in + 3 * d_in) * 2 + batch * 3 * img * img * 4 * 2
    return int(1.25 * (state + depth * per_layer + transient))


def pick_batch(d, depth, img, patch, free):
    for b in BATCHES:
        if footprint_bytes(d, depth, img, patch, b) <= free:
            return b
    return None


def make_step(cfg, batch, seed=1234):
    from fastvim_amd import fastvim as fv
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    from fastvim_amd.lr_decay import param_groups_lrd
    from fastvim_amd.mixup import Mixup
    from fastvim_amd.pipeline import SegmentedTrainStep
    factory, d, depth, img, patch, dpr = CONFIGS[cfg]
    torch.manual_seed(seed)
    model = getattr(fv, factory)(img_size=img, drop_path_rate=dpr, scaling_factor=0.25, num_classes=CLASSES).cuda().train()
    gen = torch.Generator().manual_seed(100)
    x = torch.randn(batch, 3, img, img, generator=gen).cuda()
    labels = torch.randint(0, CLASSES, (batch,), generator=gen).cuda()
    flat = FlatTrainingState(model)
    groups = param_groups_lrd(model, 0.05, no_weight_decay_list=model.no_weight_decay(), layer_decay=0.75)
    opt = FlatAdamW(flat, model, lr=1e-3, param_groups=groups, max_grad_norm=3.0, ema_decay=0.9999)
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=CLASSES)
    mix.sample()
    torch.manual_seed(5678)
    seg = SegmentedTrainStep(model, flat, opt, mix.criterion(), x, labels, n_segments=3, use_graph=True, mixup=mix)
    return seg, mix, flat, opt, sum(p.numel() for p in model.parameters())


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def kernel_table_of_step(seg, mix, steps, top):
    """[(name, calls per step, average us, share)] of the replayed step, device kernels only."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            mix.sample()
            seg.step()
        torch.cuda.synchronize()
    rows = [(e.key, e.count, getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0))
            for e in prof.key_averages()]
    rows = [r for r in rows if r[2] > 0]
    total = sum(r[2] for r in rows) or 1.0
    rows.sort(key=lambda r: -r[2])
    return [(n, c / steps, t / c, t / total) for n, c, t in rows[:top]], total / steps


def plan_of(family, batch, rows, cols, d_in, dtype_code=1):
    from fastvim_amd import _lib as L
    out = (ctypes.c_int * 8)()
    L.lib().fv_mixer_plan(L.i32(family), L.i32(batch), L.i32(rows), L.i32(cols), L.i32(1), L.i32(d_in), L.i32(0),
                          L.i32(dtype_code), out)
    form = {0: "unsupported", 1: "generic", 2: "row", 3: "cell", 4: "wave"}[out[0]]
    return f"{form} vec {out[1]} waves {out[2]} slabs {out[3]} row groups {out[4]} lds {out[5]} B"


def row_kernels(batch, grid, d, curve):
    """The four row-kernel families at (batch, grid x grid, d_inner = 2 d), bf16, HBM-cold, against the copy floor."""
    from fastvim_amd import mixer_ops as M
    dev, dt = "cuda", torch.bfloat16
    rows = cols = grid
    d_in, L_ = 2 * d, grid * grid
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s, dt_=dt: torch.randn(*s, device=dev, generator=g).to(dt_)
    f32 = torch.float32
    T = {"xz": rn(batch, L_, 2 * d_in)}
    cw, cwb = rn(d_in, 4, dt_=f32) * 0.5, rn(d_in, 4, dt_=f32) * 0.5
    cb, cbb = rn(d_in, dt_=f32) * 0.1, rn(d_in, dt_=f32) * 0.1
    D, Db = torch.ones(d_in, device=dev), torch.ones(d_in, device=dev)
    lnw, lnb = torch.ones(d_in, device=dev), torch.zeros(d_in, device=dev)
    T["xc"], T["skip"] = M.conv_pool_fwd(T["xz"], cw, cb, cwb, cbb, rows, cols, False, 0, 0.25, D=D, D_b=Db)
    T["yc"] = torch.randn(2, batch, rows, d_in, device=dev, generator=g)
    _, T["mean"], T["rstd"] = M.combine_fwd(T["xz"], T["skip"], T["yc"], lnw, lnb, 1e-5, rows, cols, False)
    T["dg"] = rn(batch, L_, d_in)
    T["dxz"] = torch.empty_like(T["xz"])
    T["d_o"], _, _ = M.combine_bwd(T["dg"], T["xz"], T["skip"], T["yc"], lnw, lnb, T["mean"], T["rstd"], T["dxz"], rows, cols, False)
    T["dxc"] = torch.randn(2, batch, rows, d_in, device=dev, generator=g)
    T["dxc2"] = rn(2, batch, rows, d_in)
    two = M.conv_pool_bwd2_ok(rows, cols, 1, d_in, False)
    U, small = batch * L_ * d_in * 2, batch * rows * d_in
    table = {   # name: (launch, rotating tensors, algorithmic bytes (the formulas of bench.py / DESIGN.md), plan family)
        "conv_pool_fwd": (lambda s: M.conv_pool_fwd(s["xz"], cw, cb, cwb, cbb, rows, cols, False, 0, 0.25, D=D, D_b=Db),
                          ("xz",), 2 * U + 2 * small * 2, 0),
        "combine_fwd": (lambda s: M.combine_fwd(s["xz"], s["skip"], s["yc"], lnw, lnb, 1e-5, rows, cols, False),
                        ("xz", "skip", "yc"), 3 * U + 2 * small * 4 + 2 * batch * L_ * 4, 1),
        "combine_bwd": (lambda s: M.combine_bwd(s["dg"], s["xz"], s["skip"], s["yc"], lnw, lnb, s["mean"], s["rstd"], s["dxz"],
                                                rows, cols, False),
                        ("dg", "xz", "skip", "yc", "mean", "rstd", "dxz"), 5 * U + 3 * small * 4 + 2 * batch * L_ * 4, 2),
        "conv_pool_bwd": (lambda s: M.conv_pool_bwd(s["xz"], s["d_o"], s["dxc"], cw, cb, cwb, cbb, D, Db, s["dxz"], rows, cols,
                                                    False, 0, 0.25, dxc2=s["dxc2"] if two else None),
                          ("xz", "d_o", "dxc", "dxz") + (("dxc2",) if two else ()), 3 * U + 2 * small * 4 + (2 * small * 2 if two else 0), 3),
    }
    out = {}
    real_reduce = M.reduce_partials      # the step defers these sums into reduce_partials_multi: not part of the row's launch
    M.reduce_partials = lambda part, n, out=None, **kw: out if out is not None else part[0]
    try:
        for name, (fn, names, nbytes, fam) in table.items():
            fns = rotating(fn, T, names, nbytes)
            us = time_kernel(fns) * 1e6
            fl = floor_us(curve, nbytes / 1e6)
            out[name] = {"us": round(us, 2), "algorithmic_MB": round(nbytes / 1e6, 2), "floor_us": round(fl, 2),
                         "floor_ratio": round(us / fl, 2), "TBps": round(nbytes / us / 1e6, 3),
                         "plan": plan_of(fam, batch, rows, cols, d_in)}
            del fns
    finally:
        M.reduce_partials = real_reduce
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="L224,H224,H448")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3, help="replayed steps per timed round")
    ap.add_argument("--top", type=int, default=24, help="rows of the per-kernel table")
    ap.add_argument("--batch", type=int, default=0, help="force a batch (0: the largest of 128 .. 8 that fits)")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--log", default=os.path.join(R, "profiles", "lh_bench.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lh.py needs a GPU")
    lines, out = [], {"rounds": args.rounds, "steps": args.steps, "configs": {}}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"{torch.cuda.get_device_name()}: fine-tuning step of FastVim-L / -H, bf16, graph replay; "
        f"{args.rounds} rounds of {args.steps} steps")
    curve = None if args.no_kernels else floor_curve(torch.bfloat16, sizes_mb=(8, 16, 32, 64, 112, 160, 320, 640))
    if curve:
        say("  copy floor (MB moved, us): " + ", ".join(f"({a:.0f}, {b:.1f})" for a, b in curve))
        out["floor_curve"] = [(round(a, 1), round(b, 2)) for a, b in curve]
    for cfg in [c for c in args.configs.split(",") if c]:
        factory, d, depth, img, patch, dpr = CONFIGS[cfg]
        grid = img // patch
        torch.cuda.empty_cache()
        free, total = torch.cuda.mem_get_info()
        batch = args.batch or pick_batch(d, depth, img, patch, free)
        rec = out["configs"][cfg] = {"d_model": d, "depth": depth, "img": img, "grid": grid, "batch": batch,
                                     "free_GB": round(free / 2**30, 1)}
        if batch is None:
            say(f"[{cfg}] no batch of {BATCHES} fits {free / 2**30:.1f} GB free: skipped")
            continue
        est = footprint_bytes(d, depth, img, patch, batch)
        say(f"[{cfg}] d_model {d}, depth {depth}, {img} px / {patch} = {grid} x {grid} tokens, drop_path {dpr}: batch {batch} "
            f"(estimated {est / 2**30:.1f} GB of {free / 2**30:.1f} GB free)")
        if not args.no_step:
            torch.cuda.reset_peak_memory_stats()
            seg, mix, flat, opt, nparam = make_step(cfg, batch)
            for _ in range(2):
                mix.sample(); seg.step()
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.rounds):
                mix.sample()
                ts.append(timed(seg.step, args.steps))
            med = statistics.median(ts)
            loss = seg.loss.item()
            peak = torch.cuda.max_memory_allocated()
            say(f"  {nparam / 1e6:.0f} M parameters; step median {med:.2f} ms (min {min(ts):.2f}, max {max(ts):.2f}) = "
                f"{batch / med * 1e3:.0f} img/s; loss {loss:.4f}, optimizer finite: {opt.last_stats()['finite']}; "
                f"peak memory {peak / 2**30:.1f} GB (estimate {est / 2**30:.1f})")
            rec.update({"params_M": round(nparam / 1e6, 1), "ms_per_step": round(med, 3), "ms_rounds": [round(t, 3) for t in ts],
                        "img_per_s": round(batch / med * 1e3, 1), "peak_GB": round(peak / 2**30, 2), "estimate_GB": round(est / 2**30, 2)})
            table, dev_ms = kernel_table_of_step(seg, mix, 2, args.top)
            say(f"  kernels of the replayed step (device time {dev_ms / 1e3:.2f} ms / step):")
            say(f"    {'kernel':<72} {'calls':>7} {'avg us':>9} {'share':>7}")
            for name, calls, avg, share in table:
                say(f"    {name[:72]:<72} {calls:7.1f} {avg:9.1f} {100 * share:6.1f}%")
            rec["kernels_of_step"] = [{"name": n, "calls": round(c, 1), "avg_us": round(a, 2), "share": round(s, 4)} for n, c, a, s in table]
            flat.close()
            del seg, mix, flat, opt
            torch.cuda.empty_cache()
        if not args.no_kernels:
            rk = row_kernels(batch, grid, d, curve)
            say(f"  mixer row kernels at batch {batch}, {grid} x {grid}, d_inner {2 * d}, HBM-cold, against a copy of the same bytes:")
            for name, v in rk.items():
                say(f"    {name:<14} {v['us']:8.1f} us  {v['algorithmic_MB']:8.1f} MB  {v['TBps']:.2f} TB/s  copy {v['floor_us']:8.1f} us  "
                    f"floor_ratio {v['floor_ratio']:.2f}   [{v['plan']}]")
            rec["row_kernels"] = rk
            torch.cuda.empty_cache()
    lines.append(json.dumps(out))
    print(lines[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
