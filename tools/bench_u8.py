"""Time the uint8 image path (fastvim_amd/pixels.py, csrc/unfold_u8.hip) on the GPU, in ONE process:

  (a) the u8 unfold kernels HBM-cold (operand sets rotated past the Infinity Cache, bench.py's ``rotating``) next to the
      float kernels they mirror, at (128, 3, 224, 224) -- plain and Mixup -- and (64, 8, 224, 224) -- per channel --, patch
      16, bf16 patches.  Every kernel is timed TWICE, so the log shows the run's own spread next to the ratios;
  (b) a pinned-memory host-to-device copy of the uint8 batch next to the fp32 batch;
  (c) the graph-replayed FastVim-T training step fed by a uint8 buffer next to the same step fed by an fp32 buffer,
      alternated in rounds.

    python tools/bench_u8.py            # --no-step: (a) and (b) only

Every GPU step runs under a time limit of its own (``--limit`` seconds): a watchdog thread ends the process with exit
code 124 if the step has not finished by then, and nothing further is started.  Reads nothing outside the repository and
sets no threshold.  The log goes to stdout and to ``--log`` (profiles/u8_bench.log), the last line one JSON record."""
import argparse
import json
import os
import statistics
import sys
import threading

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import torch  # noqa: E402
import fastvim_amd  # noqa: E402,F401  (sets the graph-capture switch before HIP initialises)
from bench import rotating, time_kernel  # noqa: E402
from fastvim_amd import glue_ops as G  # noqa: E402
from fastvim_amd.pixels import IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD, PixelNorm, attach_pixel_norm  # noqa: E402

PATCH, CLASSES = 16, 1000
MEAN8 = (0.0913, 0.1377, 0.2048, 0.0562, 0.3301, 0.4419, 0.0271, 0.1802)
STD8 = (0.0721, 0.1139, 0.1618, 0.0333, 0.2504, 0.2987, 0.0119, 0.0906)


class limited:
    """``with limited(seconds, what):`` -- the step's own time limit: past it the process ends (exit code 124)."""

    def __init__(self, seconds, what):
        self.t = threading.Timer(seconds, self._expired, (seconds, what))
        self.t.daemon = True

    @staticmethod
    def _expired(seconds, what):
        print(f"bench_u8.py: '{what}' did not finish within {seconds} s -- ending the process", flush=True)
        os._exit(124)

    def __enter__(self):
        self.t.start()

    def __exit__(self, *exc):
        self.t.cancel()


def cold_us(fn, base, names, nbytes):
    fns = rotating(fn, base, names, nbytes, cap=16)
    us = time_kernel(fns) * 1e6
    del fns
    return us


def bench_kernels(say, limit):
    rec = {}
    out_dtype = torch.bfloat16
    # ---- (128, 3, 224, 224): plain and Mixup
    shape = (128, 3, 224, 224)
    n = shape[0] * shape[1] * shape[2] * shape[3]
    pn = PixelNorm(IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD)
    table = pn.table("cuda")
    xu = torch.randint(0, 256, shape, device="cuda", dtype=torch.uint8)
    xf = pn(xu).contiguous()
    from fastvim_amd.mixup import Mixup
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, num_classes=CLASSES)
    mix.bind(xu)
    mix.set(0.3172)
    block = mix.block(xu.device)
    cases = [
        ("patch_unfold        fp32 -> bf16", lambda s: G.patch_unfold(s["x"], PATCH, PATCH, out_dtype), {"x": xf}, 4 * n + 2 * n),
        ("patch_unfold_u8     u8   -> bf16", lambda s: G.patch_unfold_u8(s["x"], table, PATCH, PATCH, out_dtype), {"x": xu}, n + 2 * n),
        ("patch_unfold_mix    fp32 -> bf16", lambda s: G.patch_unfold_mix(s["x"], PATCH, PATCH, out_dtype, block), {"x": xf}, 4 * n + 2 * n),
        ("patch_unfold_mix_u8 u8   -> bf16", lambda s: G.patch_unfold_mix_u8(s["x"], table, PATCH, PATCH, out_dtype, block), {"x": xu}, n + 2 * n),
    ]
    say(f"(a) unfold kernels, HBM-cold, {shape}, patch {PATCH} (us per launch, each kernel timed twice; MB = bytes read + written):")
    for name, fn, base, nbytes in cases:
        with limited(limit, name):
            t = [cold_us(fn, base, ("x",), nbytes) for _ in range(2)]
        rec[name.split()[0]] = {"us": [round(v, 2) for v in t], "MB": round(nbytes / 1e6, 1)}
        say(f"  {name}: {t[0]:8.2f} {t[1]:8.2f} us   {nbytes / 1e6:6.1f} MB   {nbytes / min(t) / 1e6:.2f} TB/s")
    del xu, xf
    # ---- (64, 8, 224, 224): per channel, all eight channels through the index array
    shape = (64, 8, 224, 224)
    n = shape[0] * shape[1] * shape[2] * shape[3]
    pn8 = PixelNorm(MEAN8, STD8)
    table8 = pn8.table("cuda")
    xu = torch.randint(0, 256, shape, device="cuda", dtype=torch.uint8)
    xf = pn8(xu).contiguous()
    sel = torch.arange(8, dtype=torch.int32, device="cuda")
    cases = [
        ("patch_unfold_chan    fp32 -> bf16", lambda s: G.patch_unfold_chan(s["x"], PATCH, PATCH, out_dtype, sel, 8), {"x": xf}, 4 * n + 2 * n),
        ("patch_unfold_chan_u8 u8   -> bf16", lambda s: G.patch_unfold_chan_u8(s["x"], table8, PATCH, PATCH, out_dtype, sel, 8), {"x": xu}, n + 2 * n),
    ]
    say(f"    {shape}, patch {PATCH}, 8 of 8 channels:")
    for name, fn, base, nbytes in cases:
        with limited(limit, name):
            t = [cold_us(fn, base, ("x",), nbytes) for _ in range(2)]
        rec[name.split()[0]] = {"us": [round(v, 2) for v in t], "MB": round(nbytes / 1e6, 1)}
        say(f"  {name}: {t[0]:8.2f} {t[1]:8.2f} us   {nbytes / 1e6:6.1f} MB   {nbytes / min(t) / 1e6:.2f} TB/s")
    for u8, fl in (("patch_unfold_u8", "patch_unfold"), ("patch_unfold_mix_u8", "patch_unfold_mix"), ("patch_unfold_chan_u8", "patch_unfold_chan")):
        a, b = rec[u8]["us"], rec[fl]["us"]
        ratio = statistics.mean(a) / statistics.mean(b)
        spread = max(abs(a[0] - a[1]) / min(a), abs(b[0] - b[1]) / min(b))
        rec[u8]["ratio_to_float"] = round(ratio, 3)
        rec[u8]["spread"] = round(spread, 3)
        say(f"  {u8} / {fl}: {ratio:.3f} of the float kernel's time (by bytes: 0.5); the run's own spread {100 * spread:.1f} %")
    return rec


def bench_h2d(say, limit, iters=20):
    shape = (128, 3, 224, 224)
    rec = {}
    say(f"(b) pinned host -> device copy of one {shape} batch (ms per copy, median of {iters}):")
    for name, dt in (("uint8", torch.uint8), ("fp32", torch.float32)):
        with limited(limit, "h2d " + name):
            host = torch.zeros(shape, dtype=dt).pin_memory()
            dev = torch.empty(shape, dtype=dt, device="cuda")
            dev.copy_(host, non_blocking=True)
            torch.cuda.synchronize()
            ts = []
            for _ in range(iters):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                dev.copy_(host, non_blocking=True)
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b))
        mb = host.numel() * host.element_size() / 1e6
        med = statistics.median(ts)
        rec[name] = {"ms": round(med, 4), "MB": round(mb, 1), "GBps": round(mb / med, 1)}
        say(f"  {name:5s}: {med:8.3f} ms  [{min(ts):.3f} .. {max(ts):.3f}]   {mb:6.1f} MB   {mb / med:.1f} GB/s")
    return rec


def bench_step(say, limit, steps, rounds, batch=128):
    from fastvim_amd import fastvim as fv
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    from fastvim_amd.losses import SoftTargetCrossEntropy
    from fastvim_amd.mixup import Mixup
    from fastvim_amd.pipeline import SegmentedTrainStep
    gen = torch.Generator().manual_seed(100)
    xu = torch.randint(0, 256, (batch, 3, 224, 224), generator=gen, dtype=torch.uint8).cuda()
    labels = torch.randint(0, CLASSES, (batch,), generator=gen).cuda()
    losses = {}

    # one step object at a time is alive with its FlatTrainingState (process-wide switches): build, time, close, then the other,
    # twice each in alternation
    def make(u8):
        torch.manual_seed(1234)
        model = fv.FastVimT(img_size=224, drop_path_rate=0.05).cuda().train()
        pn = attach_pixel_norm(model, IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD)
        x = xu.clone() if u8 else pn(xu).contiguous()
        flat = FlatTrainingState(model)
        no_decay = {n for n, p in model.named_parameters()
                    if p.ndim <= 1 or n.endswith(".bias") or n in model.no_weight_decay() or getattr(p, "_no_weight_decay", False)}
        opt = FlatAdamW(flat, model, lr=1e-3, weight_decay=0.05, no_decay=no_decay, ema_decay=0.9999)
        mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=CLASSES)
        mix.set(0.8)
        tgt = mix.target(labels)
        torch.manual_seed(5678)
        seg = SegmentedTrainStep(model, flat, opt, SoftTargetCrossEntropy(), x, tgt, n_segments=3)
        return seg, flat

    times = {"uint8": [], "fp32": []}
    for rnd in range(2):
        for name, u8 in (("uint8", True), ("fp32", False)):
            with limited(limit, f"step {name} round {rnd}"):
                seg, flat = make(u8)
                for _ in range(3):
                    seg.step()
                torch.cuda.synchronize()
                for _ in range(rounds):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(steps):
                        loss = seg.step()
                    b.record()
                    b.synchronize()
                    times[name].append(a.elapsed_time(b) / steps)
                losses.setdefault(name, loss.item())
                graph = seg.use_graph
                flat.close()
                del seg, flat
                torch.cuda.empty_cache()
    rec = {"batch": batch, "graph_replayed": graph, "loss_equal": losses["uint8"] == losses["fp32"]}
    say(f"(c) FastVim-T 224 px, batch {batch}, bf16, graph-replayed training step (ms per step, median [min .. max] over two "
        f"builds x {rounds} rounds of {steps}):")
    for name, v in times.items():
        rec[name + "_ms"] = [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]
        say(f"  x {name:5s}: {statistics.median(v):8.3f}  [{min(v):.3f} .. {max(v):.3f}]   {batch / statistics.median(v) * 1e3:.0f} img/s")
    say(f"  the same loss after the same steps from both buffers: {rec['loss_equal']}")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds each GPU step may take")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--log", default=os.path.join(R, "profiles", "u8_bench.log"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    assert torch.cuda.is_available(), "bench_u8.py needs a GPU"
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    rec = {"kernels": bench_kernels(say, a.limit), "h2d": bench_h2d(say, a.limit)}
    if not a.no_step:
        rec["step"] = bench_step(say, a.limit, a.steps, a.rounds)
    say(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    with open(a.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
