"""Time hierarchical channel sampling (fastvim_amd/hcs.py) on the GPU, in ONE run:

  (a)  FastChannelVim-S/16, batch 64, bf16, for every channel count 1..8: the graph-replayed step
       (``SegmentedTrainStep(..., hcs=sampler)``, the family of that count) against the EAGER step with the same subset
       (``use_graph=False``: what a model with ``hcs=True`` could run before the sampler existed), the two taking turns
       inside a round; median and spread over ``--rounds`` rounds, and the mean over the uniform count distribution --
       the step time of the real recipe
  (b)  the embed kernels against the torch chain they replace, counts 1, 4 and 8, HBM-cold: ``fv_patch_unfold_chan``
       against gather + reshape / permute / reshape copy + cast; table + ``fv_gemm_bf16_rowbias`` against ``LinearFn`` +
       the full-length epilogue add; algorithmic bytes of each
  (c)  construction of the step with its 8 families of graphs: seconds and peak device memory

    python tools/bench_hcs.py                            # everything; --no-step skips (a) and (c)
    python tools/bench_hcs.py --trace-steps 20 --count 5     # only N replayed steps at one count: the program to put under
                                                             # rocprofv3 --kernel-trace --stats

(b) runs HBM-cold the way tools/bench_mixup.py does: a case is a HIP graph of back-to-back launches cycling through
``--sets`` operand sets, every launch writing memory of its own; device time from events around a replay.  The log goes to
stdout and to ``--log`` (profiles/hcs_bench.log), the last line one JSON record."""
import argparse
import json
import os
import random
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import torch  # noqa: E402
import fastvim_amd  # noqa: E402,F401  (sets the graph-capture switch before HIP initialises)
from fastvim_amd import glue_ops as G  # noqa: E402
from fastvim_amd.hcs import ChannelSampler  # noqa: E402
from tools.bench_mixup import time_cases  # noqa: E402

BATCH, CHANNELS, IMG, PATCH, DIM, CLASSES = 64, 8, 224, 16, 384, 1000


def subset_of(count):
    """One fixed, sorted subset per count (the same for the replayed and the eager step)."""
    return sorted(random.Random(count).sample(range(CHANNELS), count))


def make_step(use_graph, seed=1234):
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    from fastvim_amd.models_channel_mamba_faster import (
        channelvim_small_patch16_224_final_pool_mean_abs_pos_embed_with_noclstok_div2 as chan_s)
    from fastvim_amd.pipeline import SegmentedTrainStep
    torch.manual_seed(seed)
    model = chan_s(img_size=IMG, channels=CHANNELS, hcs=True, drop_path_rate=0.05, num_classes=CLASSES).cuda().train()
    gen = torch.Generator().manual_seed(100)
    x = torch.randn(BATCH, CHANNELS, IMG, IMG, generator=gen).cuda()
    labels = torch.randint(0, CLASSES, (BATCH,), generator=gen).cuda()
    flat = FlatTrainingState(model)
    no_decay = {n for n, p in model.named_parameters()
                if p.ndim <= 1 or n.endswith(".bias") or n in model.no_weight_decay() or getattr(p, "_no_weight_decay", False)}
    opt = FlatAdamW(flat, model, lr=1e-3, weight_decay=0.05, no_decay=no_decay, ema_decay=0.9999)
    sampler = ChannelSampler(CHANNELS)
    torch.manual_seed(5678)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    seg = SegmentedTrainStep(model, flat, opt, torch.nn.CrossEntropyLoss(), x, labels, n_segments=3, use_graph=use_graph, hcs=sampler)
    torch.cuda.synchronize()
    build = {"seconds": time.perf_counter() - t0, "peak_MB": torch.cuda.max_memory_allocated() / 2**20,
             "before_MB": base / 2**20, "after_MB": torch.cuda.memory_allocated() / 2**20,
             "reserved_MB": torch.cuda.memory_reserved() / 2**20}
    return seg, sampler, flat, build


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
    ap.add_argument("--sets", type=int, default=6)
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5, help="(a): steps per timed round and count")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--count", type=int, default=5)
    ap.add_argument("--log", default=os.path.join(R, "profiles", "hcs_bench.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hcs.py needs a GPU")

    if args.trace_steps:
        seg, sampler, flat, _ = make_step(True)
        sampler.set(subset_of(args.count))
        for _ in range(args.trace_steps):
            loss = seg.step()
        torch.cuda.synchronize()
        print(f"{args.trace_steps} replayed steps at count {args.count} {sampler.last()}, final loss {loss.item():.5f}")
        flat.close()
        return

    lines, out = [], {"batch": BATCH, "channels": CHANNELS, "img": IMG, "rounds": args.rounds, "steps": args.steps}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"{torch.cuda.get_device_name()}: FastChannelVim-S/16, {CHANNELS} channels, {IMG} px, batch {BATCH}, bf16")

    # (b) the embed kernels against the chain they replace
    from fastvim_amd.mamba_simple_faster import LinearFn
    from fastvim_amd.models_channel_mamba_faster import _ChannelEmbedEpilogueFn, _ChanPatchProjFn
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn(BATCH, CHANNELS, IMG, IMG, device="cuda", generator=g) for _ in range(args.sets)]
    P, K = (IMG // PATCH) ** 2, PATCH * PATCH
    W = (0.05 * torch.randn(DIM, 1, 1, PATCH, PATCH, device="cuda", generator=g))
    bias, chan = torch.randn(DIM, device="cuda", generator=g), torch.randn(CHANNELS, DIM, device="cuda", generator=g)
    pos = torch.randn(1, P, DIM, device="cuda", generator=g)
    bf = torch.bfloat16

    def chain_unfold(x, ch):
        xs_ = x[:, ch, :, :]
        c = len(ch)
        return xs_.reshape(BATCH, c, IMG // PATCH, PATCH, IMG // PATCH, PATCH).permute(0, 2, 4, 1, 3, 5).reshape(BATCH, P * c, K).to(bf)

    out["kernels"] = {}
    with torch.no_grad():
        for c in (1, 4, 8):
            ch = subset_of(c)
            sel = torch.tensor(ch, dtype=torch.int32, device="cuda")
            px = BATCH * c * IMG * IMG
            M = BATCH * P * c
            pats = [G.patch_unfold_chan(x, PATCH, PATCH, bf, sel, c) for x in xs]
            cases = [
                (f"unfold_chan c={c}", [(lambda x=x: G.patch_unfold_chan(x, PATCH, PATCH, bf, sel, c)) for x in xs], px * (4 + 2)),
                # gather (read + write fp32), permuted copy (read + write fp32), cast (read fp32, write bf16)
                (f"torch chain c={c}", [(lambda x=x: chain_unfold(x, ch)) for x in xs], px * (4 + 4 + 4 + 4 + 4 + 2)),
                (f"table+gemm c={c}", [(lambda p=p: _ChanPatchProjFn.apply(p, W, bias, chan, pos, sel, c, bf)) for p in pats],
                 M * K * 2 + M * DIM * 4 + P * c * DIM * 4),
                # GEMM writes bf16 lin, the epilogue reads it back and writes fp32
                (f"linear+epilogue c={c}", [(lambda p=p: _ChannelEmbedEpilogueFn.apply(
                    LinearFn.apply(p, W, bf).view(BATCH, P, c, DIM), bias, chan[None][:, ch], pos)) for p in pats],
                 M * K * 2 + M * DIM * 2 + M * DIM * 2 + M * DIM * 4),
            ]
            times = time_cases([(n, f) for n, f, _ in cases], args.launches, args.rounds)
            for name, _, by in cases:
                ts = times[name]
                med = statistics.median(ts)
                say(f"  (b {name:<22}) {by / 1e6:7.1f} MB  median {med:8.2f} us  min {min(ts):8.2f}  max {max(ts):8.2f}  {by / med / 1e6:6.3f} TB/s")
                out["kernels"][name] = {"bytes": by, "us_median": med, "us_min": min(ts), "us_max": max(ts)}
            del pats, cases
            torch.cuda.empty_cache()
    del xs
    torch.cuda.empty_cache()

    if not args.no_step:
        # (c) construction, (a) the step per count
        seg, sampler, f0, build = make_step(True)
        say(f"  (c construction, 8 families) {build['seconds']:.1f} s; device memory {build['before_MB']:.0f} MB before, peak "
            f"{build['peak_MB']:.0f} MB, {build['after_MB']:.0f} MB after (reserved {build['reserved_MB']:.0f} MB)")
        out["construction"] = build
        eag, sampler_e, f1, _ = make_step(False)
        st = {c: {"replay": [], "eager": []} for c in range(1, CHANNELS + 1)}
        for c in st:                                     # one untimed step each
            sampler.set(subset_of(c)); sampler_e.set(subset_of(c))
            seg.step(); eag.step()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for c in st:
                sampler.set(subset_of(c)); sampler_e.set(subset_of(c))
                st[c]["replay"].append(timed(seg.step, args.steps))
                st[c]["eager"].append(timed(eag.step, args.steps))
        out["step_ms"] = {}
        worst = None
        for c, d in st.items():
            r, e = d["replay"], d["eager"]
            mr, me = statistics.median(r), statistics.median(e)
            spread = max(max(r) - min(r), max(e) - min(e))
            say(f"  (a count {c} {str(subset_of(c)):<26}) replay median {mr:8.3f} ms (min {min(r):.3f} max {max(r):.3f})   eager median "
                f"{me:8.3f} ms (min {min(e):.3f} max {max(e):.3f})   replay - eager {mr - me:+9.3f} ms, spread of the rounds {spread:.3f} ms")
            out["step_ms"][c] = {"replay_median": mr, "eager_median": me, "replay_rounds": r, "eager_rounds": e, "spread": spread}
            if worst is None or mr - me - spread > worst[1]:
                worst = (c, mr - me - spread)
        mean_r = statistics.mean(out["step_ms"][c]["replay_median"] for c in st)
        mean_e = statistics.mean(out["step_ms"][c]["eager_median"] for c in st)
        say(f"  mean over the uniform count distribution: replay {mean_r:.3f} ms / step ({BATCH / mean_r * 1e3:.0f} img/s), eager "
            f"{mean_e:.3f} ms / step; the replayed step is {'NOT ' if worst[1] > 0 else ''}within the spread of the eager one or faster "
            f"for every count (worst: count {worst[0]}, {worst[1]:+.3f} ms beyond the spread)")
        out["step_ms"]["mean_replay"], out["step_ms"]["mean_eager"] = mean_r, mean_e
        f0.close(); f1.close()
    lines.append(json.dumps(out))
    print(lines[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
