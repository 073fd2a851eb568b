"""Time random erasing (fastvim_amd/erasing.py, csrc/erase.hip, the ERASE forms of csrc/unfold_u8.hip) on the GPU, in ONE
process, at (128, 3, 224, 224) -> bf16 patches, patch 16:

  (a) HBM-cold (operand sets rotated past the Infinity Cache, bench.py's ``rotating``): ``fv_patch_unfold_u8_re`` and
      ``fv_patch_unfold_mix_u8_re`` with boxes drawn at ``probability`` 0.25 (the reference's recipes) and 1.0 (every sample
      erased) next to the plain u8 launches, and ``fv_random_erase`` on the fp32 batch, out of place and in place.  Every kernel
      is timed TWICE, so the log shows the run's own spread next to the differences;
  (b) the graph-replayed FastVim-T training step from a uint8 buffer with Mixup, with and without ``erase=``, alternated.

    python tools/bench_erase.py            # --no-step: (a) only

Every GPU step runs under a time limit of its own (``--limit`` seconds): a watchdog thread ends the process with exit
code 124 if the step has not finished by then, and nothing further is started.  Reads nothing outside the repository and
sets no threshold.  The log goes to stdout and to ``--log`` (profiles/erase_bench.log), the last line one JSON record."""
import argparse
import json
import os
import random
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))
import torch  # noqa: E402
import fastvim_amd  # noqa: E402,F401  (sets the graph-capture switch before HIP initialises)
from bench_u8 import cold_us, limited  # noqa: E402
from fastvim_amd import glue_ops as G  # noqa: E402
from fastvim_amd.erasing import RandomErasing  # noqa: E402
from fastvim_amd.mixup import Mixup  # noqa: E402
from fastvim_amd.pixels import IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD, PixelNorm, attach_pixel_norm  # noqa: E402

PATCH, CLASSES = 16, 1000
SHAPE = (128, 3, 224, 224)


def drawn(prob, x):
    """A RandomErasing bound to ``x`` with one draw at ``prob`` from a fixed generator; the fraction of erased pixels."""
    re = RandomErasing(prob, mode="pixel", max_count=1, seed=1).bind(x)
    boxes = re.sample(rng=random.Random(0))
    frac = sum(h * w for _, _, h, w in boxes) / (x.shape[0] * x.shape[2] * x.shape[3])
    return re, sum(1 for b in boxes if b[2] > 0), frac


def bench_kernels(say, limit):
    rec = {}
    out_dtype = torch.bfloat16
    n = SHAPE[0] * SHAPE[1] * SHAPE[2] * SHAPE[3]
    pn = PixelNorm(IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD)
    table = pn.table("cuda")
    xu = torch.randint(0, 256, SHAPE, device="cuda", dtype=torch.uint8)
    xf = pn(xu).contiguous()
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, num_classes=CLASSES)
    mix.bind(xu)
    mix.set(0.3172)
    mblock = mix.block(xu.device)
    re25, n25, f25 = drawn(0.25, xu)
    re100, n100, f100 = drawn(1.0, xu)
    say(f"boxes: probability 0.25 -> {n25} of {SHAPE[0]} samples, {100 * f25:.1f} % of the pixels; 1.0 -> {n100} samples, {100 * f100:.1f} %")
    b25, b100 = re25.block(), re100.block()
    cases = [
        ("patch_unfold_u8              ", lambda s: G.patch_unfold_u8(s["x"], table, PATCH, PATCH, out_dtype), {"x": xu}, 3 * n),
        ("patch_unfold_u8_re     p=0.25", lambda s: G.patch_unfold_u8_re(s["x"], table, PATCH, PATCH, out_dtype, b25), {"x": xu}, 3 * n),
        ("patch_unfold_u8_re     p=1.0 ", lambda s: G.patch_unfold_u8_re(s["x"], table, PATCH, PATCH, out_dtype, b100), {"x": xu}, 3 * n),
        ("patch_unfold_mix_u8          ", lambda s: G.patch_unfold_mix_u8(s["x"], table, PATCH, PATCH, out_dtype, mblock), {"x": xu}, 3 * n),
        ("patch_unfold_mix_u8_re p=0.25", lambda s: G.patch_unfold_mix_u8_re(s["x"], table, PATCH, PATCH, out_dtype, mblock, b25), {"x": xu}, 3 * n),
        ("patch_unfold_mix_u8_re p=1.0 ", lambda s: G.patch_unfold_mix_u8_re(s["x"], table, PATCH, PATCH, out_dtype, mblock, b100), {"x": xu}, 3 * n),
        ("random_erase fp32      p=0.25", lambda s: G.random_erase(s["x"], b25), {"x": xf}, 8 * n),
        ("random_erase fp32      p=1.0 ", lambda s: G.random_erase(s["x"], b100), {"x": xf}, 8 * n),
        ("random_erase in place  p=0.25", lambda s: G.random_erase(s["x"], b25, out=s["x"]), {"x": xf}, int(8 * n * f25)),
    ]
    say(f"(a) HBM-cold, {SHAPE}, patch {PATCH}, bf16 patches (us per launch, each kernel timed twice; MB = bytes read + written):")
    for name, fn, base, nbytes in cases:
        with limited(limit, name):
            t = [cold_us(fn, base, ("x",), max(nbytes, 3 * n)) for _ in range(2)]
        rec[" ".join(name.split())] = {"us": [round(v, 2) for v in t], "MB": round(nbytes / 1e6, 1)}
        say(f"  {name}: {t[0]:8.2f} {t[1]:8.2f} us   {nbytes / 1e6:6.1f} MB   {nbytes / min(t) / 1e6:.2f} TB/s")
    for plain in ("patch_unfold_u8", "patch_unfold_mix_u8"):
        b = rec[plain]["us"]
        for p in ("p=0.25", "p=1.0"):
            a = rec[f"{plain}_re {p}"]["us"]
            ratio = statistics.mean(a) / statistics.mean(b)
            spread = max(abs(a[0] - a[1]) / min(a), abs(b[0] - b[1]) / min(b))
            rec[f"{plain}_re {p}"]["ratio_to_plain"] = round(ratio, 3)
            rec[f"{plain}_re {p}"]["spread"] = round(spread, 3)
            say(f"  {plain}_re {p} / {plain}: {ratio:.3f} of the plain launch's time; the run's own spread {100 * spread:.1f} %")
    return rec


def bench_step(say, limit, steps, rounds, batch=128):
    from fastvim_amd import fastvim as fv
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    from fastvim_amd.pipeline import SegmentedTrainStep
    gen = torch.Generator().manual_seed(100)
    xu = torch.randint(0, 256, (batch, 3, 224, 224), generator=gen, dtype=torch.uint8).cuda()
    labels = torch.randint(0, CLASSES, (batch,), generator=gen).cuda()

    def make(erase):
        torch.manual_seed(1234)
        model = fv.FastVimT(img_size=224, drop_path_rate=0.05).cuda().train()
        attach_pixel_norm(model, IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD)
        x = xu.clone()
        flat = FlatTrainingState(model)
        no_decay = {n for n, p in model.named_parameters()
                    if p.ndim <= 1 or n.endswith(".bias") or n in model.no_weight_decay() or getattr(p, "_no_weight_decay", False)}
        opt = FlatAdamW(flat, model, lr=1e-3, weight_decay=0.05, no_decay=no_decay, ema_decay=0.9999)
        mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=CLASSES)
        mix.set(0.8)
        re = RandomErasing(0.25, mode="pixel", max_count=1, seed=0) if erase else None
        torch.manual_seed(5678)
        seg = SegmentedTrainStep(model, flat, opt, mix.criterion(), x, labels, n_segments=3, mixup=mix, erase=re)
        return seg, flat, re

    times = {"erase": [], "plain": []}
    rng = random.Random(0)
    for rnd in range(2):
        for name, erase in (("erase", True), ("plain", False)):
            with limited(limit, f"step {name} round {rnd}"):
                seg, flat, re = make(erase)
                for _ in range(3):
                    seg.step()
                torch.cuda.synchronize()
                for _ in range(rounds):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(steps):
                        if re is not None:
                            re.sample(rng=rng)      # the per-step host work of the recipe: the draw and the block's copy
                        loss = seg.step()
                    b.record()
                    b.synchronize()
                    times[name].append(a.elapsed_time(b) / steps)
                finite = bool(torch.isfinite(loss))
                graph = seg.use_graph
                flat.close()
                del seg, flat
                torch.cuda.empty_cache()
    rec = {"batch": batch, "graph_replayed": graph, "loss_finite": finite}
    say(f"(b) FastVim-T 224 px, batch {batch}, bf16, uint8 buffer, Mixup, graph-replayed training step (ms per step, median "
        f"[min .. max] over two builds x {rounds} rounds of {steps}; erase: probability 0.25, sample() before every step):")
    for name, v in times.items():
        rec[name + "_ms"] = [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]
        say(f"  {name:5s}: {statistics.median(v):8.3f}  [{min(v):.3f} .. {max(v):.3f}]   {batch / statistics.median(v) * 1e3:.0f} img/s")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds each GPU step may take")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--log", default=os.path.join(R, "profiles", "erase_bench.log"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    assert torch.cuda.is_available(), "bench_erase.py needs a GPU"
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    rec = {"kernels": bench_kernels(say, a.limit)}
    if not a.no_step:
        rec["step"] = bench_step(say, a.limit, a.steps, a.rounds)
    say(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    with open(a.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
