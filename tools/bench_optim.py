"""Time the fused optimizer's three forms at the flat sizes of FastVim-T and FastVim-B, EMA on, in ONE run, alternating:

  (i)   fv_adamw_flat                                  (adamw_flat_kernel: what an un-grouped FlatAdamW launches)
  (ii)  fv_adamw_flat_groups, 51-row table, no clip    (adamw_flat_groups_kernel)
  (iii) fv_grad_sumsq_partials + (ii) with clipping    (grad_sumsq_kernel, adamw_flat_groups_kernel, the checked step bump)
  (i')  (i) once more, on a second set of buffers      (what buffer placement alone is worth)

    python tools/bench_optim.py --size T        # or B; one size per process, so a job script can bound each with a timeout

Each case is captured as a HIP graph of ``--launches`` back-to-back steps on its OWN buffers and replayed ``--rounds``
times, the cases taking turns inside a round; device time from events around a replay.  Prints bytes moved, us per step
and TB/s per case (median and min over the rounds) and the round-to-round spread of (i), then one JSON line.
Back-to-back steps at the T size (7.2 M elements, 272 MB per step) partly live in the Infinity Cache; inside the training
step the optimizer's buffers are cold.  The B size (98 M, 3.7 GB per step) is HBM-bound either way."""
import argparse
import ctypes
import json
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import torch  # noqa: E402
import fastvim_amd  # noqa: E402,F401  (sets the graph-capture switch before HIP initialises)
from fastvim_amd import _lib as L  # noqa: E402

SIZES = {"T": 7_170_000, "B": 97_700_000}      # elements of the flat buffers (bench.py --model T / B), multiples of 8
N_GROUPS = 51                                   # param_groups_lrd on a 24-block model


class Case:
    def __init__(self, n, kind, seed):
        dev = "cuda"
        g = torch.Generator(device=dev).manual_seed(seed)
        self.n, self.kind = n, kind
        self.p = torch.randn(n, device=dev, generator=g) * 0.02
        self.g = torch.randn(n, device=dev, generator=g) * 1e-3
        self.m = torch.zeros(n, device=dev)
        self.v = torch.zeros(n, device=dev)
        self.ema = self.p.clone()
        self.shadow = torch.zeros(n, device=dev, dtype=torch.bfloat16)
        self.lr = torch.full((1,), 1e-4, device=dev)
        self.step = torch.zeros(1, device=dev)
        self.G = int(L.lib().fv_grad_sumsq_blocks(ctypes.c_size_t(n)))
        if kind == "flat":
            self.mask = torch.ones(n, device=dev, dtype=torch.uint8)
        else:
            # contiguous runs of one group, as the layer-major flat layout gives
            self.ids = (torch.arange(n, device=dev) // -(-n // N_GROUPS)).to(torch.uint8)
            self.table = torch.tensor([[0.75 ** (i // 4), 0.05 * (i % 2)] for i in range(N_GROUPS)], device=dev)
            self.partials = torch.zeros(self.G, device=dev) if kind == "clip" else None
            self.stats = torch.zeros(4, device=dev) if kind == "clip" else None
            self.max_norm = torch.full((1,), 1.0, device=dev) if kind == "clip" else None

    def bytes(self):
        n = self.n
        b = 38 * n + n                                  # p, g, m, v read; p, m, v, shadow written; EMA read + written; 1 byte of mask / group
        blocks = min(2048, -(-(n // 4) // 256))
        if self.kind != "flat":
            b += blocks * N_GROUPS * 8                  # the table, once per workgroup (L2)
        if self.kind == "clip":
            b += 4 * n + 4 * self.G + (blocks + 1) * 4 * self.G      # the norm pass; G partials per workgroup (L2)
        return b

    def run(self):
        lib, c = L.lib(), self
        st = L.stream_of(c.p)
        f = ctypes.c_float
        if c.kind == "flat":
            rc = lib.fv_adamw_flat(L.ptr(c.p), L.ptr(c.g), L.ptr(c.m), L.ptr(c.v), L.ptr(c.ema), L.ptr(c.shadow),
                                   L.ptr(c.mask), L.ptr(c.lr), L.ptr(c.step), f(0.9), f(0.999), f(1e-8), f(0.05),
                                   f(0.9999), f(1.0), ctypes.c_size_t(c.n), st)
            L.check(rc, "adamw_flat")
            return
        if c.kind == "clip":
            L.check(lib.fv_grad_sumsq_partials(L.ptr(c.g), L.ptr(c.partials), ctypes.c_size_t(c.n), st), "grad_sumsq_partials")
        rc = lib.fv_adamw_flat_groups(L.ptr(c.p), L.ptr(c.g), L.ptr(c.m), L.ptr(c.v), L.ptr(c.ema), L.ptr(c.shadow),
                                      L.ptr(c.ids), L.ptr(c.table), L.i32(N_GROUPS), L.ptr(c.lr), L.ptr(c.step),
                                      L.ptr(c.partials), L.i32(c.G if c.kind == "clip" else 0), L.ptr(c.max_norm),
                                      L.ptr(c.stats), L.i32(0), f(0.9), f(0.999), f(1e-8), f(0.9999), f(1.0),
                                      ctypes.c_size_t(c.n), st)
        L.check(rc, "adamw_flat_groups")


def capture(case, launches):
    for _ in range(3):
        case.run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            for _ in range(launches):
                case.run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="T", choices=sorted(SIZES))
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py needs a GPU")
    n = SIZES[args.size]
    # (i') is (i) again on a second set of buffers: what buffer placement alone is worth, beside the round-to-round spread
    cases = [("i   adamw_flat", Case(n, "flat", 1)), ("ii  groups", Case(n, "groups", 2)), ("iii norm+groups+clip", Case(n, "clip", 3)),
             ("i'  adamw_flat, 2nd buffers", Case(n, "flat", 4))]
    graphs = [capture(c, args.launches) for _, c in cases]
    for g in graphs:                                   # one untimed replay each
        g.replay()
    torch.cuda.synchronize()
    times = [[] for _ in cases]
    for _ in range(args.rounds):
        for k, g in enumerate(graphs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3 / args.launches)       # us per step
    out = {"size": args.size, "n": n, "launches": args.launches, "rounds": args.rounds, "G": cases[2][1].G, "cases": {}}
    print(f"size {args.size}: n = {n}, G = {cases[2][1].G} partials, {args.launches} steps per replay, {args.rounds} rounds")
    for (name, c), ts in zip(cases, times):
        med, lo, hi = statistics.median(ts), min(ts), max(ts)
        by = c.bytes()
        print(f"  ({name:<27}) {by / 1e6:9.1f} MB  median {med:9.2f} us  min {lo:9.2f} us  max {hi:9.2f} us  "
              f"{by / med / 1e6:6.3f} TB/s (median)")
        out["cases"][name.split()[0].replace("'", "2")] = {"bytes": by, "us_median": med, "us_min": lo, "us_max": hi, "tbps_median": by / med / 1e6,
                                         "us_rounds": ts}
    t1 = times[0]
    spread = (max(t1) - min(t1)) / statistics.median(t1)
    m1, m2, m3 = (statistics.median(t) for t in times[:3])
    print(f"  spread of (i) over the rounds: {100 * spread:.2f} %   (ii) - (i): {m2 - m1:+.2f} us ({100 * (m2 - m1) / m1:+.2f} %)   "
          f"(iii) - (i): {m3 - m1:+.2f} us; bytes alone, (i) x 4/38: {m1 * 4 / 38:.2f} us")
    print(f"  (i') - (i): {statistics.median(times[3]) - m1:+.2f} us")
    out.update(spread_i=spread, ii_minus_i_us=m2 - m1, iii_minus_i_us=m3 - m1, i2_minus_i_us=statistics.median(times[3]) - m1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
