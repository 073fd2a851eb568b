"""Time batch-mode Mixup / CutMix on the GPU, in ONE run, the cases taking turns:

  (a)  fv_patch_unfold                         the plain kernel, listed twice (a, a'): the run's own spread
  (b)  fv_patch_unfold_mix                     under mixup and under cutmix
  (c)  fv_mix_batch followed by fv_patch_unfold
  (d)  fv_soft_target_ce on a dense (128, 1000) target against fv_label_ce on the labels
  (e)  the FastVim-T flat-state graph step (batch 128, SegmentedTrainStep, 3 segments), mixup=None against mixup on
       (the host draws and writes new parameters before every step, as a training loop does)

    python tools/bench_mixup.py                       # everything; --no-step skips (e)
    python tools/bench_mixup.py --trace-steps 20 --mixup on      # only N replayed steps: the program to put under
                                                                  # rocprofv3 --kernel-trace --stats (fold with rocpd_stats.py)

(a)-(d) run HBM-cold: a case is a HIP graph of back-to-back launches that cycle through ``--sets`` operand sets (a set has
left the Infinity Cache when it comes round again), every launch writing memory of its own; device time from events around
a replay; median / min / max over ``--rounds`` rounds.  Shapes: (128, 3, 224, 224) fp32 images -> bf16 patches of 16 x 16.
The log goes to stdout and to ``--log`` (profiles/mixup_bench.log), the last line one JSON record."""
import argparse
import json
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import fastvim_amd  # noqa: E402,F401  (sets the graph-capture switch before HIP initialises)
from fastvim_amd import glue_ops as G  # noqa: E402
from fastvim_amd.losses import SoftTargetCrossEntropy  # noqa: E402
from fastvim_amd.mixup import Mixup  # noqa: E402

SHAPE, PATCH, CLASSES = (128, 3, 224, 224), 16, 1000


def capture(fns, launches):
    """A graph of ``launches`` back-to-back calls cycling through ``fns`` (one per operand set); results are kept alive so
    that every launch writes its own memory."""
    n = len(fns)
    for i in range(min(n, 3)):
        fns[i]()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g, keep = torch.cuda.CUDAGraph(), []
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            for i in range(launches):
                keep.append(fns[i % n]())
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    return g, keep


def time_cases(cases, launches, rounds):
    """cases: [(name, [callables])] -> {name: [us per launch, one per round]}, the cases taking turns inside a round."""
    graphs = [(name, capture(fns, launches)) for name, fns in cases]
    for _, (g, _) in graphs:
        g.replay()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in cases}
    for _ in range(rounds):
        for name, (g, _) in graphs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / launches)
    return times


def make_step(mixup_on, batch, seed=1234):
    from fastvim_amd import fastvim as fv
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    from fastvim_amd.pipeline import SegmentedTrainStep
    torch.manual_seed(seed)
    model = fv.FastVimT(img_size=224, drop_path_rate=0.05).cuda().train()
    gen = torch.Generator().manual_seed(100)
    x = torch.randn(batch, 3, 224, 224, generator=gen).cuda()
    labels = torch.randint(0, CLASSES, (batch,), generator=gen).cuda()
    flat = FlatTrainingState(model)
    no_decay = {n for n, p in model.named_parameters()
                if p.ndim <= 1 or n.endswith(".bias") or n in model.no_weight_decay() or getattr(p, "_no_weight_decay", False)}
    opt = FlatAdamW(flat, model, lr=1e-3, weight_decay=0.05, no_decay=no_decay, ema_decay=0.9999)
    torch.manual_seed(5678)
    if mixup_on:
        mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=CLASSES)
        seg = SegmentedTrainStep(model, flat, opt, mix.criterion(), x, labels, n_segments=3, mixup=mix)

        def step():
            mix.sample()
            return seg.step()
    else:
        # the parent's step: a dense soft target somebody else has mixed
        mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=CLASSES)
        mix.set(0.8)
        tgt = mix.target(labels)
        seg = SegmentedTrainStep(model, flat, opt, SoftTargetCrossEntropy(), x, tgt, n_segments=3)

        def step():
            return seg.step()
    return step, flat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=6)
    ap.add_argument("--launches", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=10, help="(e): steps per timed round")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--mixup", default="on", choices=["on", "off"])
    ap.add_argument("--log", default=os.path.join(R, "profiles", "mixup_bench.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mixup.py needs a GPU")
    np.random.seed(0)

    if args.trace_steps:
        step, flat = make_step(args.mixup == "on", SHAPE[0])
        for _ in range(args.trace_steps):
            loss = step()
        torch.cuda.synchronize()
        print(f"{args.trace_steps} replayed steps, mixup {args.mixup}, final loss {loss.item():.5f}")
        flat.close()
        return

    lines, out = [], {"shape": SHAPE, "patch": PATCH, "sets": args.sets, "launches": args.launches, "rounds": args.rounds}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"{torch.cuda.get_device_name()}: images {SHAPE} fp32 -> bf16 patches {PATCH} x {PATCH}; {args.sets} operand sets, "
        f"{args.launches} launches per replay, {args.rounds} rounds, cases interleaved")
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn(SHAPE, device="cuda", generator=g) for _ in range(args.sets)]
    H, W = SHAPE[2:]
    mix_m = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0)
    mix_m.set(0.3172)
    mix_c = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0)
    mix_c.set(0.6, use_cutmix=True, box=(30, 170, 51, 193))
    bm, bc = mix_m.block("cuda"), mix_c.block("cuda")
    in_b = xs[0].numel() * 4
    out_b = xs[0].numel() * 2
    unfold = lambda x: (lambda: G.patch_unfold(x, PATCH, PATCH, torch.bfloat16))
    cases = [
        ("a  patch_unfold", [unfold(x) for x in xs], in_b + out_b),
        ("b  patch_unfold_mix, mixup", [(lambda x=x: G.patch_unfold_mix(x, PATCH, PATCH, torch.bfloat16, bm)) for x in xs], in_b + out_b),
        ("b' patch_unfold_mix, cutmix", [(lambda x=x: G.patch_unfold_mix(x, PATCH, PATCH, torch.bfloat16, bc)) for x in xs], in_b + out_b),
        ("c  mix_batch + patch_unfold", [(lambda x=x: G.patch_unfold(G.mix_batch(x, bm), PATCH, PATCH, torch.bfloat16)) for x in xs],
         3 * in_b + out_b),
        ("c' mix_batch alone", [(lambda x=x: G.mix_batch(x, bm)) for x in xs], 2 * in_b),
        ("a' patch_unfold again", [unfold(x) for x in xs], in_b + out_b),
    ]
    times = time_cases([(n, f) for n, f, _ in cases], args.launches, args.rounds)
    out["kernels"] = {}
    for name, _, by in cases:
        ts = times[name]
        med = statistics.median(ts)
        say(f"  ({name:<28}) {by / 1e6:7.1f} MB  median {med:8.2f} us  min {min(ts):8.2f}  max {max(ts):8.2f}  {by / med / 1e6:6.3f} TB/s")
        out["kernels"][name.split()[0]] = {"bytes": by, "us_median": med, "us_min": min(ts), "us_max": max(ts), "us_rounds": ts}
    a1, a2 = statistics.median(times[cases[0][0]]), statistics.median(times[cases[5][0]])
    b1, b2, c1 = (statistics.median(times[cases[k][0]]) for k in (1, 2, 3))
    say(f"  spread of (a): |a - a'| = {abs(a1 - a2):.2f} us;  (b) - (a) = {b1 - min(a1, a2):+.2f} / {b1 - max(a1, a2):+.2f} us,  "
        f"(b') - (a) = {b2 - min(a1, a2):+.2f} / {b2 - max(a1, a2):+.2f} us;  (c) - (b) = {c1 - b1:+.2f} us")
    del xs, cases
    torch.cuda.empty_cache()

    # (d) the loss: dense target read from memory against the target built in registers
    B = SHAPE[0]
    mixl = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=CLASSES)
    mixl.set(0.3172)
    crit_d, crit_l = SoftTargetCrossEntropy(), mixl.criterion()
    logits = [torch.randn(B, CLASSES, device="cuda", generator=g).bfloat16() for _ in range(8)]
    labels = [torch.randint(0, CLASSES, (B,), device="cuda", generator=g) for _ in range(8)]
    dense = [mixl.target(l) for l in labels]
    with torch.no_grad():
        lt = time_cases([("d  soft_target_ce, dense target", [(lambda x=x, t=t: crit_d(x, t)) for x, t in zip(logits, dense)]),
                         ("d' label_ce, labels", [(lambda x=x, l=l: crit_l(x, l)) for x, l in zip(logits, labels)])],
                        args.launches, args.rounds)
    out["loss"] = {}
    for name, ts in lt.items():
        say(f"  ({name:<32}) median {statistics.median(ts):7.2f} us  min {min(ts):7.2f}  max {max(ts):7.2f}   (two kernels: rows + row sum)")
        out["loss"][name.split()[0]] = {"us_median": statistics.median(ts), "us_min": min(ts), "us_max": max(ts)}

    if not args.no_step:
        # (e) the whole step, plain and with mixup on, built the same way, taking turns
        plain, f0 = make_step(False, B)
        mixed, f1 = make_step(True, B)
        for _ in range(3):
            plain(); mixed()
        torch.cuda.synchronize()
        st = {"plain": [], "mixup": []}
        for _ in range(args.rounds):
            for name, fn in (("plain", plain), ("mixup", mixed)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.steps):
                    fn()
                b.record()
                b.synchronize()
                st[name].append(a.elapsed_time(b) / args.steps)
        out["step_ms"] = {}
        for name, ts in st.items():
            say(f"  (e  FastVim-T step, batch {B}, {name:<5}) median {statistics.median(ts):7.3f} ms  min {min(ts):7.3f}  max {max(ts):7.3f}")
            out["step_ms"][name] = {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "rounds": ts}
        say(f"  mixup - plain: {statistics.median(st['mixup']) - statistics.median(st['plain']):+.3f} ms; spread of plain over the rounds "
            f"{max(st['plain']) - min(st['plain']):.3f} ms")
        f0.close(); f1.close()
    lines.append(json.dumps(out))
    print(lines[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
