"""Measure the MAE pre-training step object (fastvim_amd/mae_step.py) and the keyed masking plan on the GPU, in ONE process,
rounds alternating between the variants:

  (a) MAE-B 224 px, batch 128, bf16, the whole step in one graph as ``bench.py --model M`` captures it, with
      ``fused_tokens`` and ``fused_loss`` on (masks from ``torch.rand`` inside the graph);
  (b) the same model through ``MAEPretrainStep(accum_iter=1)`` with ``n_segments`` 1 and 3 (forward graph | backward graphs
      | optimizer graph, masks from a ``MaskSampler``; a timed call is ``sampler.sample(); step.micro_step()``);
  (c) ``MAEPretrainStep(accum_iter=4, n_segments=3)``, reported per micro-batch (three of four calls run no optimizer);
  (d) stand-alone on HBM-cold rotated operands at (128, 14 x 14, K = 49): the keyed plan launch against the pair it
      replaces, ``torch.rand`` + ``fv_mae_mask_plan``.

    python tools/bench_mae_step.py            # --no-step / --no-kernels skip a part

Every GPU phase runs under its own time limit (a watchdog ends the process when a phase overruns: nothing else is then
started on the device).  The log goes to stdout and to ``--log`` (profiles/mae_step_bench.log), the last line one JSON
record.  Sets no threshold: it reports whether (b) lies within the spread of (a)'s own rounds."""
import argparse
import json
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))

from bench_mae_tokens import phase, timed  # noqa: E402

FACTORY, IMG = "mae_FastVim_base_dec512d2b", 224


def _state(batch):
    import torch
    from fastvim_amd import models_mae
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    torch.manual_seed(1234)
    model = getattr(models_mae, FACTORY)(img_size=IMG, fused_tokens=True, fused_loss=True).cuda().train()
    x = torch.randn(batch, 3, IMG, IMG, generator=torch.Generator().manual_seed(100)).cuda()
    flat = FlatTrainingState(model)
    no_decay = {n for n, p in model.named_parameters()
                if p.ndim <= 1 or n.endswith(".bias") or n in model.no_weight_decay() or getattr(p, "_no_weight_decay", False)}
    opt = FlatAdamW(flat, model, lr=1.5e-4 * batch / 256, betas=(0.9, 0.95), weight_decay=0.05, no_decay=no_decay, ema_decay=0.9999)
    torch.manual_seed(5678)
    return model, x, flat, opt


def single_graph(batch):
    """The step of ``bench.py --model M``: returns (call, loss of the last call, flat, keep-alive)."""
    import torch
    model, x, flat, opt = _state(batch)
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
    return graph.replay, (lambda: loss_buf.item()), flat, (graph, model, opt, x, seed, fwd_bwd)


def step_object(batch, accum_iter, n_segments):
    from fastvim_amd.mae_step import MAEPretrainStep
    from fastvim_amd.mae_tokens import MaskSampler
    model, x, flat, opt = _state(batch)
    sampler = MaskSampler(seed=0)
    step = MAEPretrainStep(model, flat, opt, x, sampler, mask_ratio=0.75, accum_iter=accum_iter, n_segments=n_segments)
    if not step.use_graph:
        raise SystemExit("bench_mae_step.py: the step fell back to eager execution (see its warning)")

    def call():
        sampler.sample()
        step.micro_step()

    return call, (lambda: step.loss.item()), flat, (step, model, opt, x, sampler)


def steps_part(batch, rounds, steps, say):
    variants = (("(a) one graph, torch.rand masks", lambda: single_graph(batch)),
                ("(b) MAEPretrainStep accum 1, 1 segment", lambda: step_object(batch, 1, 1)),
                ("(b) MAEPretrainStep accum 1, 3 segments", lambda: step_object(batch, 1, 3)),
                ("(c) MAEPretrainStep accum 4, 3 segments", lambda: step_object(batch, 4, 3)))
    built = {}
    with phase(f"MAE-B {IMG} px, batch {batch}, bf16: build + capture x {len(variants)}", 900, say):
        for name, make in variants:
            built[name] = make()
            for _ in range(4):
                built[name][0]()
    steps = 4 * max(1, steps // 4)                       # whole groups of the accum 4 variant
    ts = {name: [] for name, _ in variants}
    with phase(f"{rounds} alternating rounds of {steps} calls (micro-batches)", 600, say):
        for _ in range(rounds):
            for name, _ in variants:
                ts[name].append(timed(built[name][0], steps))
    rec = {"batch": batch, "calls_per_round": steps}
    for name, _ in variants:
        t = ts[name]
        med = statistics.median(t)
        say(f"    {name:<42} median {med:.3f} ms per micro-batch (min {min(t):.3f}, max {max(t):.3f}) = {batch / med * 1e3:.0f} "
            f"img/s; loss {built[name][1]():.6f}")
        rec[name] = {"ms_per_micro_batch": round(med, 3), "ms_rounds": [round(v, 3) for v in t]}
    a = ts[variants[0][0]]
    spread = max(a) - min(a)
    rec["a_spread_ms"] = round(spread, 3)
    for name, _ in variants[1:3]:
        d = statistics.median(ts[name]) - statistics.median(a)
        say(f"    {name} - (a) = {d:+.3f} ms; spread of (a)'s rounds {spread:.3f} ms: "
            f"{'within' if d <= spread else 'BEYOND'} the spread")
        rec[name]["minus_a_ms"] = round(d, 3)
    for name, _ in variants:
        built[name][2].close()
    return rec


def plan_part(say):
    import torch
    from bench import rotating, time_kernel
    from fastvim_amd import mae_tokens as MT
    B, H, W, K = 128, 14, 14, 49
    sampler = MT.MaskSampler(seed=0)
    sampler.sample()
    sampler.block("cuda")
    base = {"unused": torch.zeros(1, device="cuda")}
    rows = (("keyed plan (one launch)", lambda s: MT.mask_plan_keyed(sampler, B, (H, W), K)),
            ("torch.rand + plan (two launches)", lambda s: MT.mask_plan(torch.rand(B, H * W, device="cuda"), (H, W), K)),
            ("plan of a noise tensor alone", None))
    noise = {"noise": torch.rand(B, H * W, device="cuda")}
    out_bytes = B * (H * W * (8 + 4 + 4) + K * (4 * 8 + 3 * 4 + 4 * 4))          # what a plan launch writes
    res = {}
    for rep in (1, 2):
        for name, fn in rows:
            if fn is None:
                fns = rotating(lambda s: MT.mask_plan(s["noise"], (H, W), K), noise, ("noise",), B * H * W * 4 + out_bytes)
            else:
                fns = rotating(fn, base, ("unused",), out_bytes)          # (fresh outputs per launch: the writes are cold)
            us = time_kernel(fns) * 1e6
            say(f"    [{rep}] {name:<34} {us:8.2f} us")
            res[f"{name} #{rep}"] = round(us, 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=12, help="calls (micro-batches) per timed round, rounded to whole groups of 4")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--log", default=os.path.join(R, "profiles", "mae_step_bench.log"))
    args = ap.parse_args()
    import torch
    import fastvim_amd  # noqa: F401  (sets the graph-capture switch before HIP initialises)
    if not torch.cuda.is_available():
        raise SystemExit("bench_mae_step.py needs a GPU")
    lines, out = [], {}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush_log():
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")

    say(f"{torch.cuda.get_device_name()}: MAE pre-training step object and keyed masking plan")
    if not args.no_step:
        out["step"] = steps_part(args.batch, args.rounds, args.steps, say)
        torch.cuda.empty_cache()
        flush_log()
    if not args.no_kernels:
        with phase("masking plan at (128, 14 x 14, K = 49), stand-alone, HBM-cold", 300, say):
            out["plan"] = plan_part(say)
        flush_log()
    lines.append(json.dumps(out))
    print(lines[-1])
    flush_log()


if __name__ == "__main__":
    main()
