"""Measure the supervised training step of the Vim baseline (fastvim_amd/vim.py: ``VisionMamba``) through
``SegmentedTrainStep`` and its class-token launches (csrc/vim_tokens.hip, the row kernels of csrc/norm.hip) on the GPU, in
ONE process, rounds alternating between the variants.  Vim-T, 224 px, batch 128, bf16:

  (a) the single captured graph ``bench.py --model V`` replays (``fused_cls`` off: the code the model ran before);
  (b) ``SegmentedTrainStep`` with ``fused_cls`` off at ``n_segments`` 1 and 3;
  (c) ``SegmentedTrainStep`` with ``fused_cls`` on at ``n_segments`` 1 and 3;
  (d) (c) at 3 segments from a uint8 buffer (``attach_pixel_norm``) with Mixup and random erasing inside the unfold: a timed
      call is ``erase.sample(); mixup.sample(); step.step()``;
  (e) stand-alone on HBM-cold rotated operands at (128, 196, 192): each of the four launches next to the torch chain it
      replaces -- the forward chains as the model writes them, the backward chains as the plain ops autograd runs behind
      them, written out (nothing here differentiates: no autograd under the timing capture) -- and next to a plain copy of
      the same bytes (``floor_ratio`` as in bench.py).

    python tools/bench_vim_step.py            # --no-step / --no-kernels skip a part

Every GPU phase runs under its own time limit (a watchdog ends the process when a phase overruns: nothing else is then
started on the device).  The log goes to stdout and to ``--log`` (profiles/vim_step_bench.log), the last line one JSON
record.  Sets no threshold."""
import argparse
import json
import os
import random
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))

from bench_mae_tokens import phase, timed  # noqa: E402

IMG, CLASSES = 224, 1000
KERNEL_SHAPE = (128, 196, 192)            # (B, M, D)
MEAN3, STD3 = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _state(batch, fused_cls, u8=False):
    """Model, buffers and optimizer as bench.py::run_training_steps builds them for ``--model V``."""
    import torch
    from bench import build_model, soft_targets
    from fastvim_amd import pixels
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    torch.manual_seed(1234)
    model = build_model("V", IMG, 0.05).cuda().train()
    model.fused_cls = fused_cls
    gen = torch.Generator().manual_seed(100)
    if u8:
        pixels.attach_pixel_norm(model, MEAN3, STD3)
        x = torch.randint(0, 256, (batch, 3, IMG, IMG), generator=gen, dtype=torch.uint8).cuda()
        tgt = torch.randint(0, CLASSES, (batch,), generator=gen).cuda()
    else:
        x = torch.randn(batch, 3, IMG, IMG, generator=gen).cuda()
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


def segmented(batch, fused_cls, n_segments, augment=False):
    from fastvim_amd.losses import SoftTargetCrossEntropy
    from fastvim_amd.pipeline import SegmentedTrainStep
    model, x, tgt, flat, opt = _state(batch, fused_cls, u8=augment)
    mix = re = None
    crit = SoftTargetCrossEntropy()
    if augment:
        from fastvim_amd.erasing import RandomErasing
        from fastvim_amd.mixup import Mixup
        mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=CLASSES)
        mix.bind(x)
        mix.set(0.5)
        re = RandomErasing(0.25, mode="pixel", max_count=1, seed=3).bind(x)
        crit = mix.criterion()
    step = SegmentedTrainStep(model, flat, opt, crit, x, tgt, n_segments=n_segments, mixup=mix, erase=re)
    if not step.use_graph:
        raise SystemExit("bench_vim_step.py: the step fell back to eager execution (see its warning)")
    rng = random.Random(5)

    def call():
        if augment:
            re.sample(rng=rng)
            mix.sample()
        step.step()

    return call, (lambda: step.loss.item()), flat, (step, model, opt, x, tgt, mix, re)


def steps_part(batch, rounds, steps, say):
    variants = (("(a) single graph (bench.py --model V)", lambda: single_graph(batch)),
                ("(b) SegmentedTrainStep fused_cls off, 1 segment", lambda: segmented(batch, False, 1)),
                ("(b) SegmentedTrainStep fused_cls off, 3 segments", lambda: segmented(batch, False, 3)),
                ("(c) SegmentedTrainStep fused_cls on, 1 segment", lambda: segmented(batch, True, 1)),
                ("(c) SegmentedTrainStep fused_cls on, 3 segments", lambda: segmented(batch, True, 3)),
                ("(d) fused_cls on, 3 segments, uint8 + Mixup + erasing", lambda: segmented(batch, True, 3, augment=True)))
    built = {}
    with phase(f"Vim-T {IMG} px, batch {batch}, bf16: build + capture x {len(variants)}", 900, say):
        for name, make in variants:
            built[name] = make()
            for _ in range(4):
                built[name][0]()
    ts = {name: [] for name, _ in variants}
    with phase(f"{rounds} alternating rounds of {steps} steps", 600, say):
        for _ in range(rounds):
            for name, _ in variants:
                ts[name].append(timed(built[name][0], steps))
    rec = {"batch": batch, "steps_per_round": steps}
    for name, _ in variants:
        t = ts[name]
        med = statistics.median(t)
        say(f"    {name:<56} median {med:.3f} ms per step (min {min(t):.3f}, max {max(t):.3f}) = {batch / med * 1e3:.0f} img/s; "
            f"loss {built[name][1]():.6f}")
        rec[name] = {"ms_per_step": round(med, 3), "ms_rounds": [round(v, 3) for v in t]}
    names = [n for n, _ in variants]
    spread = max(max(ts[n]) - min(ts[n]) for n in names[:5])
    for other in names[1:5]:
        d = statistics.median(ts[other]) - statistics.median(ts[names[0]])
        say(f"    {other} - (a) = {d:+.3f} ms; largest spread of a variant's rounds {spread:.3f} ms: "
            f"{'beyond' if abs(d) > spread else 'within'} the spread")
        rec[other]["minus_single_graph_ms"] = round(d, 3)
    rec["largest_spread_ms"] = round(spread, 3)
    for name, _ in variants:
        built[name][2].close()
    return rec


def kernel_rows(B, M, D, curve, say):
    import torch
    from bench import floor_us, rotating, time_kernel
    from fastvim_amd import vim_tokens as VT
    from fastvim_amd.layernorm import layer_norm_fn
    p, rows = M // 2, M + 1
    g = torch.Generator().manual_seed(0)
    bf = torch.bfloat16
    T = {"y": torch.randn(B, M, D, generator=g).cuda(), "dout": torch.randn(B, rows, D, generator=g).cuda(),
         "hidden": torch.randn(B, rows, D, generator=g).to(bf).cuda(), "residual": torch.randn(B, rows, D, generator=g).cuda(),
         "dh": torch.empty(B, rows, D, dtype=bf).cuda(), "dr": torch.empty(B, rows, D).cuda()}
    cls, pos = torch.randn(1, 1, D, generator=g).cuda(), torch.randn(1, rows, D, generator=g).cuda()
    w = (1 + 0.1 * torch.randn(D, generator=g)).cuda()
    scale = torch.ones(B).cuda()
    dy = torch.randn(B, D, generator=g).to(bf).cuda()
    with torch.no_grad():
        # the saved state of one forward: what the backward launch reads
        ctx = type("Ctx", (), {"save_for_backward": lambda self, *t: setattr(self, "saved", t)})()
        VT._AddNormRowFn.forward(ctx, T["hidden"], T["residual"], w, None, 1e-5, p, scale, True)
        r, wf, _, mean, rstd, sc = ctx.saved

    cls_fwd = lambda s: VT._ClsTokensFn.forward(type("C", (), {})(), s["y"], cls, pos, p)
    cls_chain = lambda s: VT.cls_tokens_chain(s["y"], cls, pos, p)
    bctx = type("C", (), {"geo": (B, M, D, p, torch.float32, (1, 1, D), (1, rows, D))})()
    cls_bwd = lambda s: VT._ClsTokensFn.backward(bctx, s["dout"])

    def cls_bwd_chain(s):       # what autograd runs behind the chain: the add's sum over the batch, the cat's slices, the expand's sum
        d = s["dout"]
        return torch.cat((d[:, :p, :], d[:, p + 1:, :]), dim=1), d.sum(0, keepdim=True), d[:, p:p + 1, :].sum(0, keepdim=True)

    row_fwd = lambda s: VT._AddNormRowFn.forward(type("C", (), {"save_for_backward": lambda self, *t: None})(), s["hidden"],
                                                 s["residual"], w, None, 1e-5, p, scale, True)
    row_chain = lambda s: layer_norm_fn(s["hidden"], w, None, eps=1e-5, residual=s["residual"], prenorm=False,
                                        residual_in_fp32=True, is_rms_norm=True, row_scale=scale)[:, p, :]
    row_bwd = lambda s: VT.add_norm_row_backward(dy, r, wf, mean, rstd, sc, rows, p, True, bf, False, dhidden=s["dh"],
                                                 dresidual=s["dr"])
    # the whole-sequence backward behind the select: a zero fill, the scatter of B rows, the norm's adjoint over all rows
    full = {}
    with torch.no_grad():
        from fastvim_amd.layernorm import LayerNormFn
        fctx = type("Ctx", (), {"save_for_backward": lambda self, *t: setattr(self, "saved_tensors", t)})()
        LayerNormFn.forward(fctx, T["hidden"], w, None, T["residual"], 1e-5, False, True, True, scale, None)
        full["ctx"] = fctx

    def row_bwd_chain(s):
        d = torch.zeros(B, rows, D, device="cuda", dtype=bf)
        d[:, p] = dy
        return LayerNormFn.backward(full["ctx"], d)

    tok, tokh = B * rows * D * 4, B * rows * D * 2
    rows_ = (
        ("cls tokens fwd: launch", cls_fwd, ("y",), B * M * D * 4 + tok),
        ("cls tokens fwd: torch chain", cls_chain, ("y",), B * M * D * 4 + tok),
        ("cls tokens bwd: launch", cls_bwd, ("dout",), tok + B * M * D * 4),
        ("cls tokens bwd: torch adjoint chain", cls_bwd_chain, ("dout",), tok + B * M * D * 4),
        ("final norm row fwd: launch", row_fwd, ("hidden", "residual"), B * D * 12),
        ("final norm fwd: whole norm + select", row_chain, ("hidden", "residual"), tokh * 2 + tok * 2),
        ("final norm row bwd: launch", row_bwd, ("dh", "dr"), tokh + tok),
        ("final norm bwd: fill + scatter + whole adjoint", row_bwd_chain, (), tokh * 3 + tok * 2),
    )
    res = {}
    for rep in (1, 2):
        for name, fn, names, nbytes in rows_:
            us = time_kernel(rotating(fn, T, names, nbytes)) * 1e6
            fl = floor_us(curve, nbytes / 1e6)
            rec = {"us": round(us, 2), "MB": round(nbytes / 1e6, 2), "floor_us": round(fl, 2), "floor_ratio": round(us / fl, 2),
                   "TBps": round(nbytes / us / 1e6, 3)}
            say(f"    [{rep}] {name:<48} {us:8.1f} us  {nbytes / 1e6:7.1f} MB  {rec['TBps']:.2f} TB/s  copy {fl:7.1f} us  "
                f"floor_ratio {rec['floor_ratio']:.2f}")
            res[f"{name} #{rep}"] = rec
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8, help="steps per timed round")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--log", default=os.path.join(R, "profiles", "vim_step_bench.log"))
    args = ap.parse_args()
    import torch
    import fastvim_amd  # noqa: F401  (sets the graph-capture switch before HIP initialises)
    if not torch.cuda.is_available():
        raise SystemExit("bench_vim_step.py needs a GPU")
    lines, out = [], {}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush_log():
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")

    say(f"{torch.cuda.get_device_name()}: supervised Vim step through SegmentedTrainStep and its class-token launches")
    if not args.no_step:
        out["step"] = steps_part(args.batch, args.rounds, args.steps, say)
        torch.cuda.empty_cache()
        flush_log()
    if not args.no_kernels:
        from bench import floor_curve
        with phase("copy floor", 240, say):
            curve = floor_curve(torch.float32, sizes_mb=(0.5, 8, 16, 32, 64, 112))
            say("  copy floor (MB moved, us): " + ", ".join(f"({a:.1f}, {b:.1f})" for a, b in curve))
            out["floor_curve"] = [(round(a, 1), round(b, 2)) for a, b in curve]
        B, M, D = KERNEL_SHAPE
        with phase(f"class-token launches at ({B}, {M}, {D}), HBM-cold", 420, say):
            out["kernels"] = kernel_rows(B, M, D, curve, say)
        flush_log()
    lines.append(json.dumps(out))
    print(lines[-1])
    flush_log()


if __name__ == "__main__":
    main()
