"""Time MAE pre-training of the large models on the GPU, in ONE process:

    ML224  mae_FastVim_large_dec512d2b  224 px / 16  (d_model 1024, depth 48: 14 x 14 grid, 49 kept tokens)
    MH224  mae_FastVim_huge_dec512d2b   224 px / 14  (d_model 1280, depth 64: 16 x 16 grid, 64 kept tokens)

each in bf16 with the recipe bench.py --model M uses (mae/config/pretrain_FastVim{L,H}.yaml: lr 1.5e-4 x batch / 256,
betas (0.9, 0.95), weight decay 0.05, mask ratio 0.75), the whole step -- forward, loss, backward, fused AdamW + EMA --
captured into one graph.  Three parts:

  * per configuration, at the largest batch of {128, 64, 32, 16, 8} whose ESTIMATED footprint fits the free device
    memory: ms per step, images / s, and the per-kernel table of the replayed step (torch.profiler);
  * the combine forward / adjoint at (batch 64, 64 kept tokens, d_inner 2560) in its two descriptions -- ``rows x 1 x t``
    with tokens_per_patch = t, as the models call it, and the re-described grid ``rows*t x 1 x 1`` (the
    tokens_per_patch 1 kernels, one token per row) -- HBM-cold, against a plain copy kernel moving the same bytes in
    the same run (the ``floor_ratio`` of bench.py).  The shipped library launches the first as the second
    (fvplan::combine_redescribed); a library with tokens_per_patch > 1 instantiations of the 8-channel kernels shows
    their time in the first row;
  * fv_patch_unfold and fv_patch_unfold_mix at patch 14, (128, 3, 224, 224) and (64, 3, 448, 448), fp32 -> bf16,
    against the chain they replace (fv_mix_batch + torch's strided copy) and against the patch-16 kernels at
    (128, 3, 224, 224), same method.

    python tools/bench_mae_lh.py                  # --configs ML224,MH224; --no-step / --no-combine / --no-unfold skip a part

Reads nothing outside the repository and sets no threshold (the parent of these kernels cannot run MAE-H and has never
run MAE-L).  The log goes to stdout and to ``--log`` (profiles/mae_lh_bench.log), the last line one JSON record.  Give it
a time limit of its own when it runs next to other work (``timeout -k 10 900 python tools/bench_mae_lh.py``)."""
import argparse
import json
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import torch  # noqa: E402
import fastvim_amd  # noqa: E402,F401  (sets the graph-capture switch before HIP initialises)
from bench import floor_curve, floor_us, rotating, time_kernel  # noqa: E402

BATCHES = (128, 64, 32, 16, 8)
#          name: (factory, d_model, depth, img, patch)
CONFIGS = {
    "ML224": ("mae_FastVim_large_dec512d2b", 1024, 48, 224, 16),
    "MH224": ("mae_FastVim_huge_dec512d2b", 1280, 64, 224, 14),
}
MASK = 0.75


def mixer_params(d):
    d_in, R_, N = 2 * d, -(-d // 16), 16
    return 2 * d_in * d + d * d_in + 2 * d_in + 2 * (d_in * N + d_in + d_in * 5 + (R_ + 2 * N) * d_in + d_in * R_ + d_in)


def footprint_bytes(d, depth, img, patch, batch):
    """Estimated device bytes of the replayed step at ``batch``: the flat training state (fp32 parameters, gradients, two
    Adam moments, EMA; bf16 shadows) and what autograd keeps per layer in bf16 storage -- for the encoder on the kept
    quarter of the tokens, for the two decoder blocks (width 512) on all of them --, the patches, the prediction and
    the images.  x 1.25 for the graph's private pool and allocator slack."""
    tokens = (img // patch) ** 2
    kept = int(tokens * (1 - MASK))
    n = depth * (mixer_params(d) + d) + 2 * (mixer_params(512) + 512) + d * 3 * patch * patch + d * 512 + 512 * 3 * patch * patch
    state = n * (5 * 4 + 2 * 2)
    enc = batch * kept * (d * (4 + 2 + 2) + 4 * (2 * d) * 2 + 2 * (2 * d) * 4)
    dec = batch * tokens * (512 * (4 + 2 + 2) + 4 * 1024 * 2)
    io = batch * (3 * img * img * (4 + 2) + tokens * 3 * patch * patch * 4 * 3)
    return int(1.25 * (state + depth * enc + 2 * dec + io))


def pick_batch(d, depth, img, patch, free):
    for b in BATCHES:
        if footprint_bytes(d, depth, img, patch, b) <= free:
            return b
    return None


def make_step(cfg, batch):
    """The captured pre-training step, built as bench.py builds the MAE-B one; returns (replay, loss buffer, flat, n)."""
    from fastvim_amd import models_mae
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    factory, d, depth, img, patch = CONFIGS[cfg]
    torch.manual_seed(1234)
    model = getattr(models_mae, factory)(img_size=img).cuda().train()
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
            loss = model(x, mask_ratio=MASK)[0]
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
    return graph.replay, loss_buf, flat, sum(p.numel() for p in model.parameters())


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def kernel_table_of_step(replay, steps, top):
    """[(name, calls per step, average us, share)] of the replayed step, device kernels only."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            replay()
        torch.cuda.synchronize()
    rows = [(e.key, e.count, getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0))
            for e in prof.key_averages()]
    rows = [r for r in rows if r[2] > 0]
    total = sum(r[2] for r in rows) or 1.0
    rows.sort(key=lambda r: -r[2])
    return [(n, c / steps, t / c, t / total) for n, c, t in rows[:top]], total / steps


def cold(fn, T, names, nbytes, curve):
    fns = rotating(fn, T, names, nbytes)
    us = time_kernel(fns) * 1e6
    fl = floor_us(curve, nbytes / 1e6)
    return {"us": round(us, 2), "MB": round(nbytes / 1e6, 2), "floor_us": round(fl, 2), "floor_ratio": round(us / fl, 2),
            "TBps": round(nbytes / us / 1e6, 3)}


def combine_launches(batch, rows, t, d_in, curve):
    """Both launches of the un-pooled combine at (batch, rows * t tokens, d_in), bf16.  Bytes: the storage-dtype
    full-length tensors (3U forward: z, skip, g; 5U adjoint: dg, z, skip, dz, d_o) and the fp32 scan rows, which in this
    geometry are full length as well (yc both directions read: 4U; adjoint also writes dyc: 2U) and the statistics."""
    from fastvim_amd import mixer_ops as M
    dev, dt = "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    Ltok = rows * t
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)
    T = {"xz": rn(batch, Ltok, 2 * d_in).to(dt), "skip": rn(batch, Ltok, d_in).to(dt), "yc": rn(2, batch, Ltok, d_in),
         "dg": rn(batch, Ltok, d_in).to(dt)}
    lnw, lnb = torch.ones(d_in, device=dev), torch.zeros(d_in, device=dev)
    _, T["mean"], T["rstd"] = M.combine_fwd(T["xz"], T["skip"], T["yc"], lnw, lnb, 1e-5, rows, 1, False, tpp=t)
    T["dxz"] = torch.empty_like(T["xz"])
    U, stats = batch * Ltok * d_in * 2, 2 * batch * Ltok * 4
    out = {}
    real_reduce = M.reduce_partials      # the step defers these sums into reduce_partials_multi: not part of the row's launch
    M.reduce_partials = lambda part, n, out=None, **kw: out if out is not None else part[0]
    try:
        for name, (r, tpp) in (("rows x 1 x t", (rows, t)), ("rows*t x 1 x 1", (Ltok, 1))):
            out[f"combine_fwd {name}"] = cold(
                lambda s: M.combine_fwd(s["xz"], s["skip"], s["yc"], lnw, lnb, 1e-5, r, 1, False, tpp=tpp),
                T, ("xz", "skip", "yc"), 3 * U + 4 * U + stats, curve)
            out[f"combine_bwd {name}"] = cold(
                lambda s: M.combine_bwd(s["dg"], s["xz"], s["skip"], s["yc"], lnw, lnb, s["mean"], s["rstd"], s["dxz"], r, 1, False, tpp=tpp),
                T, ("dg", "xz", "skip", "yc", "mean", "rstd", "dxz"), 5 * U + 4 * U + 2 * U + stats, curve)
    finally:
        M.reduce_partials = real_reduce
    return out


def unfold_rows(shape, patch, curve):
    """fv_patch_unfold / fv_patch_unfold_mix against mix_batch + the strided copy, fp32 images -> bf16 patches."""
    from fastvim_amd import glue_ops as G
    from fastvim_amd.mixup import Mixup
    B, C, H, W = shape
    gh, gw = H // patch, W // patch
    T = {"x": torch.randn(shape, device="cuda")}
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0)
    mix.bind(T["x"])
    mix.set(0.3172)
    blk = mix.block("cuda")
    nbytes = B * C * H * W * (4 + 2)

    def copy_path(x):
        patches = torch.empty(B, gh * gw, C * patch * patch, device="cuda", dtype=torch.bfloat16)
        patches.view(B, gh, gw, C, patch, patch).copy_(x.reshape(B, C, gh, patch, gw, patch).permute(0, 2, 4, 1, 3, 5))
        return patches

    out = {"patch_unfold": cold(lambda s: G.patch_unfold(s["x"], patch, patch, torch.bfloat16), T, ("x",), nbytes, curve),
           "patch_unfold_mix": cold(lambda s: G.patch_unfold_mix(s["x"], patch, patch, torch.bfloat16, blk), T, ("x",), nbytes, curve),
           "strided copy": cold(lambda s: copy_path(s["x"]), T, ("x",), nbytes, curve),
           "mix_batch + strided copy": cold(lambda s: copy_path(G.mix_batch(s["x"], blk)), T, ("x",), nbytes + B * C * H * W * 8, curve)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="ML224,MH224")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3, help="replayed steps per timed round")
    ap.add_argument("--top", type=int, default=24, help="rows of the per-kernel table")
    ap.add_argument("--batch", type=int, default=0, help="force a batch (0: the largest of 128 .. 8 that fits)")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-combine", action="store_true")
    ap.add_argument("--no-unfold", action="store_true")
    ap.add_argument("--log", default=os.path.join(R, "profiles", "mae_lh_bench.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mae_lh.py needs a GPU")
    lines, out = [], {"rounds": args.rounds, "steps": args.steps, "configs": {}}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"{torch.cuda.get_device_name()}: MAE pre-training step of FastVim-L / -H, bf16, graph replay; "
        f"{args.rounds} rounds of {args.steps} steps")
    curve = floor_curve(torch.bfloat16, sizes_mb=(8, 16, 32, 64, 112, 160, 320, 640))
    say("  copy floor (MB moved, us): " + ", ".join(f"({a:.0f}, {b:.1f})" for a, b in curve))
    out["floor_curve"] = [(round(a, 1), round(b, 2)) for a, b in curve]
    for cfg in [c for c in args.configs.split(",") if c and not args.no_step]:
        factory, d, depth, img, patch = CONFIGS[cfg]
        grid = img // patch
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info()
        batch = args.batch or pick_batch(d, depth, img, patch, free)
        rec = out["configs"][cfg] = {"factory": factory, "d_model": d, "depth": depth, "img": img, "grid": grid, "batch": batch,
                                     "free_GB": round(free / 2**30, 1)}
        if batch is None:
            say(f"[{cfg}] no batch of {BATCHES} fits {free / 2**30:.1f} GB free: skipped")
            continue
        est = footprint_bytes(d, depth, img, patch, batch)
        say(f"[{cfg}] {factory}: d_model {d}, depth {depth}, {img} px / {patch} = {grid} x {grid} tokens, "
            f"{int(grid * grid * (1 - MASK))} kept: batch {batch} (estimated {est / 2**30:.1f} GB of {free / 2**30:.1f} GB free)")
        torch.cuda.reset_peak_memory_stats()
        replay, loss_buf, flat, nparam = make_step(cfg, batch)
        for _ in range(2):
            replay()
        torch.cuda.synchronize()
        ts = [timed(replay, args.steps) for _ in range(args.rounds)]
        med = statistics.median(ts)
        peak = torch.cuda.max_memory_allocated()
        say(f"  {nparam / 1e6:.0f} M parameters; step median {med:.2f} ms (min {min(ts):.2f}, max {max(ts):.2f}) = "
            f"{batch / med * 1e3:.0f} img/s; loss {loss_buf.item():.4f}; peak memory {peak / 2**30:.1f} GB (estimate {est / 2**30:.1f})")
        rec.update({"params_M": round(nparam / 1e6, 1), "ms_per_step": round(med, 3), "ms_rounds": [round(t, 3) for t in ts],
                    "img_per_s": round(batch / med * 1e3, 1), "peak_GB": round(peak / 2**30, 2), "estimate_GB": round(est / 2**30, 2)})
        table, dev_ms = kernel_table_of_step(replay, 2, args.top)
        say(f"  kernels of the replayed step (device time {dev_ms / 1e3:.2f} ms / step):")
        say(f"    {'kernel':<72} {'calls':>7} {'avg us':>9} {'share':>7}")
        for name, calls, avg, share in table:
            say(f"    {name[:72]:<72} {calls:7.1f} {avg:9.1f} {100 * share:6.1f}%")
        rec["kernels_of_step"] = [{"name": n, "calls": round(c, 1), "avg_us": round(a, 2), "share": round(s, 4)} for n, c, a, s in table]
        flat.close()
        del replay, loss_buf, flat
        torch.cuda.empty_cache()
    if not args.no_combine:
        rk = out["combine_2560"] = combine_launches(64, 16, 4, 2560, curve)
        say("combine at batch 64, 64 kept tokens (16 rows x 4), d_inner 2560, bf16, HBM-cold, against a copy of the same bytes:")
        for name, v in rk.items():
            say(f"    {name:<28} {v['us']:8.1f} us  {v['MB']:8.1f} MB  {v['TBps']:.2f} TB/s  copy {v['floor_us']:8.1f} us  "
                f"floor_ratio {v['floor_ratio']:.2f}")
        torch.cuda.empty_cache()
    if not args.no_unfold:
        out["unfold"] = {}
        for shape, patch in (((128, 3, 224, 224), 14), ((64, 3, 448, 448), 14), ((128, 3, 224, 224), 16)):
            rk = out["unfold"][f"{shape} / {patch}"] = unfold_rows(shape, patch, curve)
            say(f"patch unfold {shape}, patch {patch}, fp32 -> bf16, HBM-cold, against a copy of the same bytes:")
            for name, v in rk.items():
                say(f"    {name:<28} {v['us']:8.1f} us  {v['MB']:8.1f} MB  {v['TBps']:.2f} TB/s  copy {v['floor_us']:8.1f} us  "
                    f"floor_ratio {v['floor_ratio']:.2f}")
            torch.cuda.empty_cache()
    lines.append(json.dumps(out))
    print(lines[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
