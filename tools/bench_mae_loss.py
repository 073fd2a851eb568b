"""Measure the fused MAE reconstruction loss (csrc/mae_loss.hip) on the GPU, in ONE process:

  * accuracy: for every case of tests/mae_loss_ref.py (shapes x pred dtype x norm_pix x mask) the error of the EXISTING
    eager fp32 composition (``forward_loss`` and its autograd) and of the fused kernels against the fp64 restatement --
    relative loss error and max|dpred - ref| / max|ref| -- and their maxima per (patch, dtype): the numbers the test
    tolerances are taken from (4 x the composition's error; + 2^-8 for bf16 dpred);
  * kernels: at pred (128, 196, 768) [224 px / 16] and (128, 256, 588) [224 px / 14], bf16 pred, 75 % removed, HBM-cold with
    rotated operands: the fused forward (two launches) and backward, from fp32 and from uint8 images, next to the eager
    composition (forward without autograd; forward + backward) and to a plain copy of the fused kernels' own bytes
    (``floor_ratio`` as in bench.py), everything twice;
  * step: the graph-replayed MAE-B pre-training step (batch 128, bf16, built as tools/bench_mae_lh.py::make_step builds it)
    with ``fused_loss`` off, on, and from a uint8 input buffer, rounds alternating between the three.

    python tools/bench_mae_loss.py            # --no-accuracy / --no-kernels / --no-step skip a part

Every GPU phase runs under its own time limit (a watchdog ends the process when a phase overruns: nothing else is then
started on the device).  The log goes to stdout and to ``--log`` (profiles/mae_loss_bench.log), the last line one JSON
record.  Sets no threshold."""
import argparse
import contextlib
import faulthandler
import json
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import torch  # noqa: E402
import fastvim_amd  # noqa: E402,F401  (sets the graph-capture switch before HIP initialises)
from bench import floor_curve, floor_us, rotating, time_kernel  # noqa: E402
import mae_loss_ref as REF  # noqa: E402

KERNEL_SHAPES = ((16, 224, 128), (14, 224, 128))       # (patch, px, batch): pred (128, 196, 768) and (128, 256, 588)


@contextlib.contextmanager
def phase(name, seconds, say):
    say(f"== {name} (time limit {seconds} s)")
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
        torch.cuda.synchronize()
    finally:
        faulthandler.cancel_dump_traceback_later()


# ------------------------------------------------------------------------------------------------ accuracy
def accuracy(say):
    from fastvim_amd.losses import _MAELossFn
    worst = {}
    rows = []
    for patch, px, N in REF.SHAPES:
        c = {k: v.cuda() for k, v in REF.make_case(patch, px, N).items()}
        for bf16 in (False, True):
            for norm_pix in (True, False):
                for mk in REF.MASKS:
                    ref, mask = REF.reference(patch, px, N, bf16, norm_pix, mk)
                    pred = c["pred"].bfloat16() if bf16 else c["pred"]
                    le, de = REF.eager_composition(c["f32"], pred, mask.cuda(), patch, norm_pix)
                    e_eager = REF.errors(le, de, ref)
                    e_fused = {}
                    for src in ("f32", "u8"):
                        pr = pred.clone().requires_grad_(True)
                        loss, _, _ = _MAELossFn.apply(pr, c[src], mask.cuda(), c["table"] if src == "u8" else None, patch, norm_pix)
                        loss.backward()
                        e_fused[src] = REF.errors(loss.detach(), pr.grad, ref)
                    assert e_fused["f32"] == e_fused["u8"], "the uint8 form differs from the float form"
                    dt = "bf16" if bf16 else "fp32"
                    rows.append({"patch": patch, "px": px, "N": N, "dtype": dt, "norm_pix": norm_pix, "mask": mk,
                                 "eager": e_eager, "fused": e_fused["f32"]})
                    say(f"  patch {patch:2d} {px:3d} px N {N} {dt} norm {int(norm_pix)} {mk:<16} eager loss {e_eager[0]:.3e} dpred "
                        f"{e_eager[1]:.3e} | fused loss {e_fused['f32'][0]:.3e} dpred {e_fused['f32'][1]:.3e}")
                    w = worst.setdefault((patch, dt), {"eager": [0.0, 0.0], "fused": [0.0, 0.0]})
                    for i in range(2):
                        w["eager"][i] = max(w["eager"][i], e_eager[i])
                        w["fused"][i] = max(w["fused"][i], e_fused["f32"][i])
    say("  maxima per (patch, dtype); bound = 4 x eager (+ 2^-8 on dpred for bf16):")
    out = {}
    for (patch, dt), w in sorted(worst.items()):
        bl, bd = 4 * w["eager"][0], 4 * w["eager"][1] + (2.0 ** -8 if dt == "bf16" else 0.0)
        say(f"    patch {patch:2d} {dt}: eager loss {w['eager'][0]:.3e} dpred {w['eager'][1]:.3e} | fused loss {w['fused'][0]:.3e} "
            f"dpred {w['fused'][1]:.3e} | bound loss {bl:.3e} dpred {bd:.3e} | within: {w['fused'][0] <= bl and w['fused'][1] <= bd}")
        out[f"{patch}/{dt}"] = {"eager": w["eager"], "fused": w["fused"], "bound": [bl, bd]}
    return {"cases": rows, "per_patch_dtype": out}


# ------------------------------------------------------------------------------------------------ kernels
def kernel_rows(patch, px, N, curve, say):
    from fastvim_amd import _lib as L
    Lp, D = (px // patch) ** 2, 3 * patch * patch
    g = torch.Generator().manual_seed(0)
    pn = REF.pixel_norm()
    u8 = torch.randint(0, 256, (N, 3, px, px), generator=g, dtype=torch.uint8).cuda()
    table = pn.table("cuda")
    mask = REF.make_mask("ratio75", N, Lp).cuda()
    T = {"f32": pn(u8), "u8": u8, "pred": torch.randn(N, Lp, D, generator=g).bfloat16().cuda()}
    T["dpred"] = torch.empty_like(T["pred"])
    rows_ = torch.empty(N, Lp, device="cuda")
    stats = torch.empty(N, Lp, 2, device="cuda")
    out2 = torch.empty(2, device="cuda")
    gone = torch.ones(1, device="cuda")
    lib, i32, p_ = L.lib(), L.i32, L.ptr
    removed = mask.sum().item() / mask.numel()

    def fwd(s, src):
        rc = lib.fv_mae_loss_fwd(p_(s[src]), p_(table if src == "u8" else None), p_(s["pred"]), i32(L.FV_BF16), p_(mask), p_(rows_),
                                 p_(stats), p_(out2), i32(N), i32(px), i32(px), i32(patch), i32(1), L.stream_of(mask))
        L.check(rc, "mae_loss_fwd")

    def bwd(s, src):
        rc = lib.fv_mae_loss_bwd(p_(s[src]), p_(table if src == "u8" else None), p_(s["pred"]), i32(L.FV_BF16), p_(mask), p_(stats),
                                 p_(out2[1:]), p_(gone), p_(s["dpred"]), i32(N), i32(px), i32(px), i32(patch), L.stream_of(mask))
        L.check(rc, "mae_loss_bwd")

    def eager_fwd(s):
        with torch.no_grad():
            t = s["f32"].reshape(N, 3, px // patch, patch, px // patch, patch).permute(0, 2, 4, 3, 5, 1).reshape(N, Lp, D)
            t = (t - t.mean(dim=-1, keepdim=True)) / (t.var(dim=-1, keepdim=True) + 1.0e-6) ** 0.5
            return ((((s["pred"] - t) ** 2).mean(dim=-1)) * mask).sum() / mask.sum()

    def eager_fwd_bwd(s):
        return REF.eager_composition(s["f32"], s["pred"], mask, patch, True)

    small = 4 * N * Lp * 4                                   # mask, loss_rows, row_stats
    nb = {src: removed * N * Lp * D * (esz + 2) + small for src, esz in (("f32", 4), ("u8", 1))}
    res = {}
    fwd(T, "f32")                                            # row_stats / sum(mask) for the backward rows
    for rep in (1, 2):
        for name, fn, names, nbytes in (
                ("fused fwd fp32 img", lambda s: fwd(s, "f32"), ("f32", "pred"), nb["f32"]),
                ("fused fwd uint8 img", lambda s: fwd(s, "u8"), ("u8", "pred"), nb["u8"]),
                ("fused bwd fp32 img", lambda s: bwd(s, "f32"), ("f32", "pred", "dpred"), nb["f32"] + N * Lp * D * 2),
                ("fused bwd uint8 img", lambda s: bwd(s, "u8"), ("u8", "pred", "dpred"), nb["u8"] + N * Lp * D * 2),
                ("eager fwd (no autograd)", eager_fwd, ("f32", "pred"), None),
                ("eager fwd + bwd", eager_fwd_bwd, ("f32", "pred"), None)):
            rot_bytes = nbytes if nbytes else N * Lp * D * 6
            us = time_kernel(rotating(fn, T, names, rot_bytes)) * 1e6
            rec = {"us": round(us, 2)}
            if nbytes:
                fl = floor_us(curve, nbytes / 1e6)
                rec.update({"MB": round(nbytes / 1e6, 2), "floor_us": round(fl, 2), "floor_ratio": round(us / fl, 2),
                            "TBps": round(nbytes / us / 1e6, 3)})
                say(f"    [{rep}] {name:<26} {us:8.1f} us  {nbytes / 1e6:7.1f} MB  {rec['TBps']:.2f} TB/s  copy {fl:7.1f} us  "
                    f"floor_ratio {rec['floor_ratio']:.2f}")
            else:
                say(f"    [{rep}] {name:<26} {us:8.1f} us")
            res[f"{name} #{rep}"] = rec
    return res


# ------------------------------------------------------------------------------------------------ step
def make_step(batch, fused_loss, u8):
    """tools/bench_mae_lh.py::make_step for mae_FastVim_base_dec512d2b at 224 px, with the loss switch and the input type;
    returns (replay, loss buffer, flat, keep-alive)."""
    from fastvim_amd import models_mae
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    from fastvim_amd.pixels import IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD, attach_pixel_norm
    torch.manual_seed(1234)
    model = models_mae.mae_FastVim_base_dec512d2b(img_size=224, fused_loss=fused_loss).cuda().train()
    pn = attach_pixel_norm(model, IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD)
    xb = torch.randint(0, 256, (batch, 3, 224, 224), generator=torch.Generator().manual_seed(100), dtype=torch.uint8).cuda()
    x = xb if u8 else pn(xb)
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
    # A captured graph holds ADDRESSES, not references: everything it reads or writes that lives outside its private pool
    # -- the input buffer, the backward seed, the optimizer's moments -- must outlive it, or the next variant's build is
    # handed that memory while this graph still writes to it.  The caller keeps the whole tuple.
    return graph.replay, loss_buf, flat, (graph, model, opt, x, xb, seed, fwd_bwd)


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10, help="replayed steps per timed round")
    ap.add_argument("--no-accuracy", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--log", default=os.path.join(R, "profiles", "mae_loss_bench.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mae_loss.py needs a GPU")
    lines, out = [], {}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush_log():
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")

    say(f"{torch.cuda.get_device_name()}: fused MAE reconstruction loss")
    if not args.no_accuracy:
        with phase("accuracy against the fp64 restatement (tests/mae_loss_ref.py)", 240, say):
            out["accuracy"] = accuracy(say)
        flush_log()
    if not args.no_kernels:
        with phase("copy floor", 240, say):
            curve = floor_curve(torch.bfloat16, sizes_mb=(8, 16, 32, 64, 112, 160))
            say("  copy floor (MB moved, us): " + ", ".join(f"({a:.0f}, {b:.1f})" for a, b in curve))
            out["floor_curve"] = [(round(a, 1), round(b, 2)) for a, b in curve]
        out["kernels"] = {}
        for patch, px, N in KERNEL_SHAPES:
            Lp, D = (px // patch) ** 2, 3 * patch * patch
            with phase(f"kernels at pred ({N}, {Lp}, {D}) bf16, {px} px / {patch}, 75 % removed, HBM-cold", 300, say):
                out["kernels"][f"({N}, {Lp}, {D})"] = kernel_rows(patch, px, N, curve, say)
            torch.cuda.empty_cache()
            flush_log()
    if not args.no_step:
        variants = (("fused_loss off, fp32 input", False, False), ("fused_loss on, fp32 input", True, False),
                    ("uint8 input (fused loss)", True, True))
        steps = {}
        with phase(f"MAE-B step, batch {args.batch}, bf16, graph replay: build + capture x 3", 420, say):
            for name, fl, u8 in variants:
                steps[name] = make_step(args.batch, fl, u8)
                for _ in range(2):
                    steps[name][0]()
        ts = {name: [] for name, _, _ in variants}
        with phase(f"MAE-B step: {args.rounds} alternating rounds of {args.steps} replays", 300, say):
            for _ in range(args.rounds):
                for name, _, _ in variants:
                    ts[name].append(timed(steps[name][0], args.steps))
        out["step"] = {}
        for name, _, _ in variants:
            med = statistics.median(ts[name])
            say(f"    {name:<28} median {med:.3f} ms (min {min(ts[name]):.3f}, max {max(ts[name]):.3f}) = "
                f"{args.batch / med * 1e3:.0f} img/s; loss {steps[name][1].item():.4f}")
            out["step"][name] = {"ms_per_step": round(med, 3), "ms_rounds": [round(t, 3) for t in ts[name]]}
        for name, _, _ in variants:
            steps[name][2].close()
    lines.append(json.dumps(out))
    print(lines[-1])
    flush_log()


if __name__ == "__main__":
    main()
