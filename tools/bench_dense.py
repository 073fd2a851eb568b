"""Time the dense-prediction kernels (csrc/chan_ln.hip) on the GPU, in ONE process, alternating rounds:

  * the feature tap at (2, 4096, C) and (2, 1024, C), C in {192, 384, 768}, fp32 hidden states, forward and backward,
    against the torch composition it replaces (``nn.LayerNorm``, ``view``, ``permute``, ``contiguous`` and its autograd
    mirror) and against a plain copy moving the same algorithmic bytes (``floor_ratio`` = time / copy time, the
    convention of bench.py's rows);
  * LN2d at (2, 256, 256, 256), (2, 256, 64, 64), (2, 96, 128, 128) and (1024, 256, 7, 7), fp32 and bf16, forward and
    backward, against the eager chain of the reference's formula (written out below) and the same copy floor;
  * eager forward + backward of ``MM_FastVim`` in the detection-T configuration (1024 px, B = 2, ``out_indices=[23]``)
    and the segmentation-B configuration (512 px, B = 2, four taps), bf16 autocast, each with the fused taps and with
    the torch composition forced.

    python tools/bench_dense.py            # --no-model: the operators only; --no-graph: eager timings only

Every candidate of a group is timed once per round, the rounds alternate between them, and the log gives the median
and the spread (min .. max) over the rounds.  The operators are timed twice: with the calls of a round replayed from one
HIP graph (device time: a single eager call of these sizes is shorter than the host work that launches it) and issued
eagerly from Python (what an eager training loop pays, host included).  The backbones run eagerly.  Calls run back to
back: a tensor set below the 256 MiB Infinity Cache can be served from it, the copy floor of the same bytes runs under the same condition.  Bytes are computed from shapes.
Fails without a GPU; reads nothing outside the repository.  The log goes to stdout and to ``--log``
(profiles/dense_bench.log), the last line one JSON record.  Give it a time limit of its own next to other work."""
import argparse
import json
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import torch  # noqa: E402
import fastvim_amd  # noqa: E402,F401  (sets the graph-capture switch before HIP initialises)

DEV = "cuda"


def graphed(fn, iters):
    """``iters`` calls of ``fn`` captured into one HIP graph (after three eager calls on a side stream): replaying it
    leaves the host out, so the events around a replay time the device."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    return g.replay


def alternating(cands, iters, rounds, graph=True):
    """{name: (median, min, max) ms per call}: every round times each candidate once -- ``iters`` calls between two
    events, replayed from a HIP graph (``graph``) or issued eagerly (then the host's share is in the number)."""
    if graph:
        runs = {k: graphed(fn, iters) for k, fn in cands.items()}
    else:
        def loop(fn):
            def run():
                for _ in range(iters):
                    fn()
            return run
        runs = {k: loop(fn) for k, fn in cands.items()}
    for run in runs.values():              # warm-up: code objects, allocator, the graph's first replay
        run()
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for _ in range(rounds):
        for k, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / iters)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def copy_of(nbytes):
    """A plain copy that moves ``nbytes`` in total (half read, half written)."""
    n = max(1, nbytes // 8)
    src, dst = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    return lambda: dst.copy_(src)


def report(say, title, res, nbytes, floor_key="copy floor"):
    say(title + f"  [{nbytes / 1e6:.1f} MB algorithmic]")
    fl = res[floor_key][0]
    out = {}
    for k, (m, lo, hi) in res.items():
        say(f"    {k:28s} {m * 1e3:9.1f} us  [{lo * 1e3:.1f} .. {hi * 1e3:.1f}]  floor_ratio {m / fl:5.2f}  {nbytes / m / 1e9:7.3f} TB/s")
        out[k] = {"us": round(m * 1e3, 2), "min_us": round(lo * 1e3, 2), "max_us": round(hi * 1e3, 2), "floor_ratio": round(m / fl, 2)}
    out["algorithmic_MB"] = round(nbytes / 1e6, 2)
    return out


def torch_tap(h, norm, H, W):
    return norm(h.float()).view(-1, H, W, h.shape[-1]).permute(0, 3, 1, 2).contiguous()


def ln2d_eager(x, weight, bias, eps):
    """The reference's formula (detection/vitdet/simple_fpn.py:27-32), op by op."""
    u = x.mean(1, keepdim=True)
    s = (x - u).pow(2).mean(1, keepdim=True)
    x = (x - u) / torch.sqrt(s + eps)
    return weight[:, None, None] * x + bias[:, None, None]


def bench_taps(iters, rounds, say, graph):
    from fastvim_amd.dense_ops import tap_layer_norm_nchw
    out = {}
    for L_, (H, W) in ((4096, (64, 64)), (1024, (32, 32))):
        for C in (192, 384, 768):
            B = 2
            norm = torch.nn.LayerNorm(C).to(DEV)
            h = torch.randn(B, L_, C, device=DEV, requires_grad=True)
            g = torch.randn(B, C, H, W, device=DEV)
            n = B * L_ * C
            fwd_bytes = n * 4 + n * 4 + 2 * B * L_ * 4                # x in, y out, mean / rstd
            bwd_bytes = 3 * n * 4 + 2 * B * L_ * 4                    # dy, x in, dx out (partial rows: (B L / 32) C floats)
            yf, yt = tap_layer_norm_nchw(h, norm.weight, norm.bias, H, W, norm.eps), torch_tap(h, norm, H, W)

            def bwd(y):
                def run():
                    h.grad = norm.weight.grad = norm.bias.grad = None
                    y.backward(g, retain_graph=True)
                return run
            key = f"tap B{B} L{L_} C{C} fp32"
            with torch.no_grad():
                res = alternating({"fused (1 launch)": lambda: tap_layer_norm_nchw(h, norm.weight, norm.bias, H, W, norm.eps),
                                   "torch composition": lambda: torch_tap(h, norm, H, W), "copy floor": copy_of(fwd_bytes)}, iters, rounds, graph)
            out[key + " fwd"] = report(say, key + " forward", res, fwd_bytes)
            res = alternating({"fused (1 launch + 2 sums)": bwd(yf), "torch autograd": bwd(yt), "copy floor": copy_of(bwd_bytes)}, iters, rounds, graph)
            out[key + " bwd"] = report(say, key + " backward", res, bwd_bytes)
    return out


def bench_ln2d(iters, rounds, say, graph):
    from fastvim_amd.dense_ops import ln2d_fn
    out = {}
    for shape in ((2, 256, 256, 256), (2, 256, 64, 64), (2, 96, 128, 128), (1024, 256, 7, 7)):
        for dt in (torch.float32, torch.bfloat16):
            N, C, H, W = shape
            w = torch.nn.Parameter(1 + 0.1 * torch.randn(C, device=DEV))
            b = torch.nn.Parameter(0.1 * torch.randn(C, device=DEV))
            x = torch.randn(*shape, device=DEV).to(dt).requires_grad_()
            g = torch.randn(*shape, device=DEV).to(dt)
            n, es = x.numel(), x.element_size()
            fwd_bytes = 2 * n * es + 2 * N * H * W * 4
            bwd_bytes = 3 * n * es + 2 * N * H * W * 4
            yf, ye = ln2d_fn(x, w, b, 1e-6), ln2d_eager(x, w, b, 1e-6)

            def bwd(y):
                def run():
                    x.grad = w.grad = b.grad = None
                    y.backward(g.to(y.dtype), retain_graph=True)
                return run
            key = f"ln2d {shape} {'bf16' if dt == torch.bfloat16 else 'fp32'}"
            it = max(2, iters // 4) if n > 2 ** 24 else iters
            with torch.no_grad():
                res = alternating({"fused (1 launch)": lambda: ln2d_fn(x, w, b, 1e-6), "eager chain": lambda: ln2d_eager(x, w, b, 1e-6),
                                   "copy floor": copy_of(fwd_bytes)}, it, rounds, graph)
            out[key + " fwd"] = report(say, key + " forward", res, fwd_bytes)
            res = alternating({"fused (1 launch + 2 sums)": bwd(yf), "eager autograd": bwd(ye), "copy floor": copy_of(bwd_bytes)}, it, rounds, graph)
            out[key + " bwd"] = report(say, key + " backward", res, bwd_bytes)
            del x, g, yf, ye
            torch.cuda.empty_cache()
    return out


def bench_backbones(iters, rounds, say):
    from fastvim_amd.fastvim import MM_FastVim
    mm = dict(patch_size=16, stride=16, rms_norm=False, fused_add_norm=False, residual_in_fp32=True, final_pool_type="all",
              if_abs_pos_embed=True, rotate_every_block=True, drop_path_rate=0.0)
    out = {}
    for name, kw in (("detection-T 1024 px [23]", dict(img_size=1024, embed_dim=192, depth=24, out_indices=[23])),
                     ("segmentation-B 512 px [5, 11, 17, 23]", dict(img_size=512, embed_dim=768, depth=24, out_indices=[5, 11, 17, 23]))):
        torch.manual_seed(0)
        m = MM_FastVim(**mm, **kw).to(DEV).train()
        x = torch.randn(2, 3, kw["img_size"], kw["img_size"], device=DEV)

        def step(fused):
            def run():
                m._fused_taps = (lambda outs: False) if not fused else type(m)._fused_taps.__get__(m)
                m.zero_grad(set_to_none=True)
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    outs = m(x)
                outs = [outs] if torch.is_tensor(outs) else outs
                sum(o.float().square().mean() for o in outs).backward()
            return run
        res = alternating({"fused taps": step(True), "torch composition": step(False)}, iters, rounds, graph=False)
        say(f"MM_FastVim {name}, B = 2, bf16 autocast, eager forward + backward (ms, median [min .. max]):")
        for k, (md, lo, hi) in res.items():
            say(f"    {k:28s} {md:9.3f}  [{lo:.3f} .. {hi:.3f}]")
        out[name] = {k: [round(v, 3) for v in t] for k, t in res.items()}
        del m, x
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--no-graph", action="store_true", help="skip the graph-replayed timings of the operators")
    ap.add_argument("--log", default=os.path.join(R, "profiles", "dense_bench.log"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    assert torch.cuda.is_available(), "bench_dense.py needs a GPU"
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {a.rounds} alternating rounds of {a.iters} calls")
    rec = {}
    for graph, tag in ((True, "graph-replayed"), (False, "eager"))[int(a.no_graph):]:
        say(f"== operators, {tag}: " + ("the calls of a round replayed from one HIP graph, device time" if graph else
                                        "issued from Python, the host's launch work included") + " ==")
        rec[tag] = {"taps": bench_taps(a.iters, a.rounds, say, graph), "ln2d": bench_ln2d(a.iters, a.rounds, say, graph)}
    if not a.no_model:
        rec["backbones"] = bench_backbones(max(2, a.iters // 5), a.rounds, say)
    say(json.dumps(rec))
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    with open(a.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
