"""Measure the training step of the ChannelVim baseline (fastvim_amd/models_channel_mamba.py: ``VisionMamba``) through
``SegmentedTrainStep`` and its class-token launches (csrc/chan_tokens.hip) on the GPU, in ONE process, rounds alternating
between the variants.  ChannelVim-S/16, 224 px, 8 channels, batch 64, bf16:

  (a) the single captured graph ``bench.py --model CV`` replays (``fused_cls`` off, no sampler: the code the model ran before);
  (b) ``SegmentedTrainStep`` with ``fused_cls`` off at ``n_segments`` 1 and 3;
  (c) ``SegmentedTrainStep`` with ``fused_cls`` on at ``n_segments`` 1 and 3;
  (d) (c) at 3 segments with ``hcs=sampler``: the family of every channel count 1..8, and their mean -- what a step of the
      recipe costs on average, the counts being drawn uniformly;
  (e) stand-alone on HBM-cold rotated operands at (64, 1568, 384) fp32 (what the patch projection hands the model): each
      of the two launches next to the torch chain it replaces -- forward as the model writes it, backward as the plain ops
      autograd runs behind it, written out -- and next to a plain copy of the same bytes (``floor_ratio`` as in bench.py).

    python tools/bench_channelvim_step.py            # --no-step / --no-kernels skip a part; --variants a,c3,d picks

The variants of (a)-(d) are alive together (alternating rounds need them to be); each holds the activations of its own
graphs.  Before a variant is built the free device memory is compared with what the first one took: a variant that would
not fit is left out and reported as such, nothing is then measured for it.  Every GPU phase runs under its own time limit (a
watchdog ends the process when a phase overruns: nothing else is then started on the device).  The log goes to stdout and to
``--log`` (profiles/channelvim_step_bench.log), the last line one JSON record.  Sets no threshold."""
import argparse
import json
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))

from bench_mae_tokens import phase, timed  # noqa: E402

IMG, CLASSES, CHANNELS = 224, 1000, 8
KERNEL_SHAPE = (64, 1568, 384)            # (B, M, D): 196 patches x 8 channels


def _state(batch, fused_cls, sample=False):
    """Model, buffers and optimizer as bench.py::run_training_steps builds them for ``--model CV``."""
    import torch
    from bench import build_model, soft_targets
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    torch.manual_seed(1234)
    model = build_model("CV", IMG, 0.1, CHANNELS).cuda().train()
    model.fused_cls = fused_cls
    model.patch_embed.hcs = bool(sample)           # (bench.py builds it with hcs off: every channel, the config's L)
    gen = torch.Generator().manual_seed(100)
    x = torch.randn(batch, CHANNELS, IMG, IMG, generator=gen).cuda()
    tgt = soft_targets(batch, CLASSES, gen, "cuda")
    flat = FlatTrainingState(model)
    no_decay = {n for n, p in model.named_parameters()
                if p.ndim <= 1 or n.endswith(".bias") or n in model.no_weight_decay() or getattr(p, "_no_weight_decay", False)}
    opt = FlatAdamW(flat, model, lr=1e-3, weight_decay=0.05, no_decay=no_decay, ema_decay=0.9999)
    torch.manual_seed(5678)
    return model, x, tgt, flat, opt


def single_graph(batch):
    """bench.py's world-1 step: forward, backward and optimizer in one captured graph."""
    import torch
    from fastvim_amd.losses import SoftTargetCrossEntropy
    model, x, tgt, flat, opt = _state(batch, False)
    crit, seed = SoftTargetCrossEntropy(), torch.ones((), device="cuda", dtype=torch.float32)

    def fwd_bwd():
        flat.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits = model(x)
        loss = crit(logits, tgt)
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
    return graph.replay, (lambda: loss_buf.item()), flat, (graph, model, opt, x, tgt, seed, fwd_bwd)


def segmented(batch, fused_cls, n_segments, sample=False):
    from fastvim_amd.hcs import ChannelSampler
    from fastvim_amd.losses import SoftTargetCrossEntropy
    from fastvim_amd.pipeline import SegmentedTrainStep
    model, x, tgt, flat, opt = _state(batch, fused_cls, sample)
    sampler = ChannelSampler(CHANNELS) if sample else None
    step = SegmentedTrainStep(model, flat, opt, SoftTargetCrossEntropy(), x, tgt, n_segments=n_segments, hcs=sampler)
    if not step.use_graph:
        raise SystemExit("bench_channelvim_step.py: the step fell back to eager execution (see its warning)")
    return step.step, (lambda: step.loss.item()), flat, (step, model, opt, x, tgt, sampler)


VARIANT_KEYS = ("a", "b1", "b3", "c1", "c3", "d")


def steps_part(batch, rounds, steps, say, keys=VARIANT_KEYS):
    import torch
    A = "(a) single graph (bench.py --model CV)"
    SAMPLED = "(d) fused_cls on, 3 segments, hcs= sampler"
    table = {"a": (A, lambda: single_graph(batch)),
             "b1": ("(b) SegmentedTrainStep fused_cls off, 1 segment", lambda: segmented(batch, False, 1)),
             "b3": ("(b) SegmentedTrainStep fused_cls off, 3 segments", lambda: segmented(batch, False, 3)),
             "c1": ("(c) SegmentedTrainStep fused_cls on, 1 segment", lambda: segmented(batch, True, 1)),
             "c3": ("(c) SegmentedTrainStep fused_cls on, 3 segments", lambda: segmented(batch, True, 3)),
             "d": (SAMPLED, lambda: segmented(batch, True, 3, sample=True))}
    variants = tuple(table[k] for k in VARIANT_KEYS if k in keys)
    built, left_out, took = {}, [], None
    with phase(f"ChannelVim-S/16 {IMG} px, {CHANNELS} channels, batch {batch}, bf16: build + capture x {len(variants)}", 1200, say):
        for name, make in variants:
            free0 = torch.cuda.mem_get_info()[0]
            if took is not None and free0 < 1.1 * took:
                say(f"    {name}: NOT BUILT -- {free0 / 2 ** 30:.1f} GiB free, the first variant took {took / 2 ** 30:.1f} GiB")
                left_out.append(name)
                continue
            built[name] = make()
            for _ in range(3):
                built[name][0]()
            torch.cuda.synchronize()
            used = free0 - torch.cuda.mem_get_info()[0]
            took = used if took is None else max(took, used)
            say(f"    {name}: built, {used / 2 ** 30:.1f} GiB")
    names = [n for n, _ in variants if n in built]
    plain = [n for n in names if n != SAMPLED]
    ts = {n: [] for n in plain}
    per_count = {c: [] for c in range(1, CHANNELS + 1)}
    with phase(f"{rounds} alternating rounds of {steps} steps", 900, say):
        for _ in range(rounds):
            for n in plain:
                ts[n].append(timed(built[n][0], steps))
            if SAMPLED in built:
                sampler = built[SAMPLED][3][5]
                for c in per_count:
                    sampler.set(range(c))
                    per_count[c].append(timed(built[SAMPLED][0], steps))
    rec = {"batch": batch, "steps_per_round": steps, "not_built": left_out}
    for n in plain:
        t = ts[n]
        med = statistics.median(t)
        say(f"    {n:<52} median {med:.3f} ms per step (min {min(t):.3f}, max {max(t):.3f}) = {batch / med * 1e3:.0f} img/s; "
            f"loss {built[n][1]():.6f}")
        rec[n] = {"ms_per_step": round(med, 3), "ms_rounds": [round(v, 3) for v in t]}
    spread = max(max(ts[n]) - min(ts[n]) for n in plain)
    rec["largest_spread_ms"] = round(spread, 3)
    if A in built:
        for other in plain[1:]:
            d = statistics.median(ts[other]) - statistics.median(ts[A])
            say(f"    {other} - (a) = {d:+.3f} ms; largest spread of a variant's rounds {spread:.3f} ms: "
                f"{'beyond' if abs(d) > spread else 'within'} the spread")
            rec[other]["minus_single_graph_ms"] = round(d, 3)
    if SAMPLED in built:
        meds = {c: statistics.median(t) for c, t in per_count.items()}
        for c, med in meds.items():
            say(f"    {SAMPLED}, {c} channel{'s' if c > 1 else ' '} ({196 * c + 1:4d} tokens)  median {med:8.3f} ms per step "
                f"(min {min(per_count[c]):.3f}, max {max(per_count[c]):.3f})")
        mean = sum(meds.values()) / len(meds)
        say(f"    {SAMPLED}, mean over the counts 1..{CHANNELS}: {mean:.3f} ms per step = {batch / mean * 1e3:.0f} img/s")
        rec[SAMPLED] = {"ms_per_step_by_count": {str(c): round(v, 3) for c, v in meds.items()}, "mean_ms_per_step": round(mean, 3),
                        "ms_rounds_by_count": {str(c): [round(v, 3) for v in t] for c, t in per_count.items()}}
    for n in names:
        built[n][2].close()
    return rec


def kernel_rows(B, M, D, curve, say):
    import torch
    from bench import floor_us, rotating, time_kernel
    from fastvim_amd import chan_tokens as CT
    p, rows = M // 2, M + 1
    g = torch.Generator().manual_seed(0)
    T = {"y": torch.randn(B, M, D, generator=g).cuda(), "dout": torch.randn(B, rows, D, generator=g).cuda(),
         "out": torch.empty(B, rows, D).cuda(), "dy": torch.empty(B, M, D).cuda()}
    cls = torch.randn(1, 1, D, generator=g).cuda()
    fwd = lambda s: CT._ChanClsTokensFn.forward(type("C", (), {})(), s["y"], cls, p)
    chain = lambda s: CT.chan_cls_tokens_chain(s["y"], cls, p)
    bctx = type("C", (), {"geo": (B, M, D, p, torch.float32, (1, 1, D))})()
    bwd = lambda s: CT._ChanClsTokensFn.backward(bctx, s["dout"])

    def bwd_chain(s):           # what autograd runs behind the chain: the cat's two slices copied out, the expand's sum over the batch
        d = s["dout"]
        return d[:, :p, :].contiguous(), d[:, p:p + 1, :].sum(0, keepdim=True), d[:, p + 1:, :].contiguous()

    def bwd_chain_one(s):       # the same adjoint written as ONE cat (fewer launches than autograd makes): the kinder yardstick
        d = s["dout"]
        return torch.cat((d[:, :p, :], d[:, p + 1:, :]), dim=1), d[:, p:p + 1, :].sum(0, keepdim=True)

    copy_fwd = lambda s: s["out"].view(-1)[:B * M * D].copy_(s["y"].view(-1))
    copy_bwd = lambda s: s["dy"].view(-1).copy_(s["dout"].view(-1)[:B * M * D])
    moved = 2 * B * M * D * 4
    rows_ = (("chan cls tokens fwd: launch", fwd, ("y",), moved),
             ("chan cls tokens fwd: torch chain", chain, ("y",), moved),
             ("chan cls tokens fwd: plain copy of the bytes", copy_fwd, ("y", "out"), moved),
             ("chan cls tokens bwd: launch", bwd, ("dout",), moved),
             ("chan cls tokens bwd: torch adjoint (slices + sum)", bwd_chain, ("dout",), moved),
             ("chan cls tokens bwd: torch adjoint (one cat + sum)", bwd_chain_one, ("dout",), moved),
             ("chan cls tokens bwd: plain copy of the bytes", copy_bwd, ("dout", "dy"), moved))
    res = {}
    for rep in (1, 2):
        for name, fn, names, nbytes in rows_:
            us = time_kernel(rotating(fn, T, names, nbytes)) * 1e6
            fl = floor_us(curve, nbytes / 1e6)
            rec = {"us": round(us, 2), "MB": round(nbytes / 1e6, 2), "floor_us": round(fl, 2), "floor_ratio": round(us / fl, 2),
                   "TBps": round(nbytes / us / 1e6, 3)}
            say(f"    [{rep}] {name:<52} {us:8.1f} us  {nbytes / 1e6:7.1f} MB  {rec['TBps']:.2f} TB/s  copy floor {fl:7.1f} us  "
                f"floor_ratio {rec['floor_ratio']:.2f}")
            res[f"{name} #{rep}"] = rec
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4, help="steps per timed round")
    ap.add_argument("--variants", default=",".join(VARIANT_KEYS),
                    help="which of (a)-(d) to build next to each other: a,b1,b3,c1,c3,d (digits: n_segments).  One variant "
                         "holds about 57 GiB at batch 64: all six do not fit one MI355X, e.g. a,b1,b3,c1 and a,c3,d do")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--log", default=os.path.join(R, "profiles", "channelvim_step_bench.log"))
    args = ap.parse_args()
    import torch
    import fastvim_amd  # noqa: F401  (sets the graph-capture switch before HIP initialises)
    if not torch.cuda.is_available():
        raise SystemExit("bench_channelvim_step.py needs a GPU")
    lines, out = [], {}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush_log():
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")

    say(f"{torch.cuda.get_device_name()}: ChannelVim step through SegmentedTrainStep and its class-token launches")
    if not args.no_kernels:                       # (first: small, and its buffers are gone before the steps are built)
        from bench import floor_curve
        with phase("copy floor", 240, say):
            curve = floor_curve(torch.float32, sizes_mb=(16, 64, 160, 320, 400))
            say("  copy floor (MB moved, us): " + ", ".join(f"({a:.1f}, {b:.1f})" for a, b in curve))
            out["floor_curve"] = [(round(a, 1), round(b, 2)) for a, b in curve]
        B, M, D = KERNEL_SHAPE
        with phase(f"class-token launches at ({B}, {M}, {D}) fp32, HBM-cold", 420, say):
            out["kernels"] = kernel_rows(B, M, D, curve, say)
        torch.cuda.empty_cache()
        flush_log()
    if not args.no_step:
        keys = tuple(k for k in args.variants.split(",") if k)
        if not set(keys) <= set(VARIANT_KEYS):
            raise SystemExit(f"--variants takes {','.join(VARIANT_KEYS)}")
        out["step"] = steps_part(args.batch, args.rounds, args.steps, say, keys)
        torch.cuda.empty_cache()
        flush_log()
    lines.append(json.dumps(out))
    print(lines[-1])
    flush_log()


if __name__ == "__main__":
    main()
