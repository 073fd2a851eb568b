"""Time the linear-probe recipe (mae/config/linear_FastVimL.yaml) on the GPU, in ONE process: FastVim-L 224 px, bf16,
the largest batch of {512, 256, 128, 64} whose estimated footprint fits the free device memory.

  * the graph-replayed probe step (``LinearProbeStep``: frozen backbone under no_grad, BatchNorm, head, loss, head
    backward, ``FlatSGD``), with ``freeze_shadows``;
  * a graph-replayed ``no_grad`` forward (features only) of the same model and batch -- what the step cannot be faster
    than; the difference is the head's share: the BatchNorm launches, two small GEMMs, the loss and the optimizer;
  * the same forward WITHOUT ``freeze_shadows`` (every frozen projection weight re-cast on every forward);
  * the new kernels stand-alone at the recipe's shapes (B x d features, a 1000 x d head): fv_bn1d_stats, fv_bn1d_apply,
    fv_bn1d_bwd, fv_sgd_flat, fv_lars_sumsq_partials + fv_lars_flat.

    python tools/bench_linear_probe.py            # --batch N forces a batch; --no-model times the kernels only

Reads nothing outside the repository and sets no threshold (the parent cannot run the recipe: there is no number to
compare with).  The log goes to stdout and to ``--log`` (profiles/linear_probe_bench.log), the last line one JSON record.
Give it a time limit of its own when it runs next to other work (``timeout -k 10 600 python tools/bench_linear_probe.py``)."""
import argparse
import json
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import torch  # noqa: E402
import fastvim_amd  # noqa: E402,F401  (sets the graph-capture switch before HIP initialises)

CLASSES, D, DEPTH, IMG, PATCH = 1000, 1024, 48, 224, 16
BATCHES = (512, 256, 128, 64)


def footprint_bytes(batch):
    """Estimated device bytes of the frozen forward at ``batch``: fp32 parameters + bf16 copies, the input, and the
    transients of ONE block (nothing is kept for backward): fp32 residual, bf16 rows, xz, conv / scan / gate rows.  x 2 for
    the graphs' private pools (three graphs are alive at once) and allocator slack."""
    d_in = 2 * D
    params = DEPTH * (3 * d_in * D + 12 * d_in * 16) + CLASSES * D
    tok = batch * (IMG // PATCH) ** 2
    block = tok * (D * (4 + 4 + 2 + 2) + 2 * d_in * 2 + 4 * d_in * 2)
    return int(2 * (params * 6 + batch * 3 * IMG * IMG * 4 + 3 * block))


def timed(fn, iters, rounds):
    """Median and spread (ms) over ``rounds`` rounds of ``iters`` calls, events around each round."""
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return statistics.median(out), min(out), max(out)


def captured_forward(model, x):
    """A graph of ``model.forward_features(x)`` under no_grad and bf16 autocast (two eager runs first)."""
    def run():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return model.forward_features(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run()
    return g, out


def bench_model(batch, steps, rounds, say):
    from fastvim_amd import fastvim as fv
    from fastvim_amd.flat import FlatSGD, FlatTrainingState
    from fastvim_amd.linear_probe import LinearProbeStep, attach_probe_head, freeze_shadows
    torch.manual_seed(1234)
    model = fv.vim_large_patch16_224_final_pool_mean_abs_pos_embed_with_noclstok_div2(img_size=IMG, num_classes=CLASSES)
    model = attach_probe_head(model).cuda().train()
    gen = torch.Generator().manual_seed(100)
    x = torch.randn(batch, 3, IMG, IMG, generator=gen).cuda()
    labels = torch.randint(0, CLASSES, (batch,), generator=gen).cuda()
    rec = {"batch": batch}
    g, _ = captured_forward(model, x)
    rec["forward_no_shadows_ms"] = timed(g.replay, steps, rounds)
    del g
    buf = freeze_shadows(model)
    rec["frozen_shadow_MB"] = round(buf.numel() * 2 / 2 ** 20, 1)
    g, _ = captured_forward(model, x)
    rec["forward_ms"] = timed(g.replay, steps, rounds)
    del g
    flat = FlatTrainingState(model)
    opt = FlatSGD(flat, model, lr=0.1, momentum=0.9, weight_decay=0.0)
    step = LinearProbeStep(model, flat, opt, x, labels)
    rec["graph_replayed"] = bool(step.use_graph)
    rec["probe_step_ms"] = timed(step.step, steps, rounds)
    rec["final_loss"] = float(step.loss)
    flat.close()
    f, s, n = rec["forward_ms"][0], rec["probe_step_ms"][0], rec["forward_no_shadows_ms"][0]
    rec["head_share_ms"] = round(s - f, 4)
    rec["img_per_s"] = round(batch / s * 1e3, 1)
    say(f"FastVim-L {IMG} px, batch {batch}, bf16 (median [min .. max] ms over {rounds} rounds of {steps}):")
    for k in ("probe_step_ms", "forward_ms", "forward_no_shadows_ms"):
        m, lo, hi = rec[k]
        say(f"  {k:24s} {m:9.3f}  [{lo:.3f} .. {hi:.3f}]")
    say(f"  head share (step - forward) {s - f:.3f} ms; frozen shadows save {n - f:.3f} ms per forward "
        f"({rec['frozen_shadow_MB']} MB of bf16 copies); {rec['img_per_s']} img/s; loss {rec['final_loss']:.4f}")
    return rec


def bench_kernels(batch, iters, rounds, say):
    """The new kernels at (batch, D) bf16 features and a (CLASSES, D) head, each timed back to back (L2-warm: the
    features of a probe step were just written by the pooling kernel)."""
    from fastvim_amd.flat import FlatSGD, FlatTrainingState
    from fastvim_amd.linear_probe import bn1d_apply, bn1d_bwd, bn1d_stats
    out = {}
    x = torch.randn(batch, D, device="cuda").to(torch.bfloat16)
    dy = torch.randn(batch, D, device="cuda").to(torch.bfloat16)
    row = torch.empty(2 * D + 1, device="cuda")
    rm, rv = torch.zeros(D, device="cuda"), torch.ones(D, device="cuda")
    nbt = torch.zeros((), dtype=torch.int64, device="cuda")
    bn1d_stats(x, row)
    _, mean, rstd = bn1d_apply(x, row, rm, rv, nbt, 1e-6, 0.1, True)
    out["fv_bn1d_stats"] = timed(lambda: bn1d_stats(x, row), iters, rounds)
    out["fv_bn1d_apply"] = timed(lambda: bn1d_apply(x, row, rm, rv, nbt, 1e-6, 0.1, True), iters, rounds)
    out["fv_bn1d_bwd"] = timed(lambda: bn1d_bwd(dy, x, mean, rstd, True), iters, rounds)
    head = torch.nn.Linear(D, CLASSES).cuda()
    with FlatTrainingState(head) as flat:
        flat.grad_flat.normal_()
        sgd = FlatSGD(flat, head, lr=1e-3)
        lars = FlatSGD(flat, head, lr=1e-3, lars=True, weight_decay=0.05)
        out["fv_sgd_flat"] = timed(sgd.step, iters, rounds)
        out["fv_lars (2 launches)"] = timed(lars.step, iters, rounds)
    say(f"kernels at B = {batch}, d = {D}, head {CLASSES} x {D} (host launch included; us, median [min .. max]):")
    for k, (m, lo, hi) in out.items():
        say(f"  {k:24s} {m * 1e3:8.1f}  [{lo * 1e3:.1f} .. {hi * 1e3:.1f}]")
    return {k: [round(v * 1e3, 2) for v in t] for k, t in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--log", default=os.path.join(R, "profiles", "linear_probe_bench.log"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    assert torch.cuda.is_available(), "bench_linear_probe.py needs a GPU"
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    rec = {}
    batch = a.batch
    if batch is None:
        free = torch.cuda.mem_get_info()[0]
        batch = next((b for b in BATCHES if footprint_bytes(b) <= free), None)
        say(f"free device memory {free / 2 ** 30:.1f} GiB; estimated footprints "
            + ", ".join(f"{b}: {footprint_bytes(b) / 2 ** 30:.1f} GiB" for b in BATCHES) + f" -> batch {batch}")
    if batch is None:
        say("no batch of 512 .. 64 fits: nothing timed")
    else:
        if not a.no_model:
            rec["model"] = bench_model(batch, a.steps, a.rounds, say)
        rec["kernels_us"] = bench_kernels(batch, 50, a.rounds, say)
    say(json.dumps(rec))
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    with open(a.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
