"""in_proj forward at the FastVim-T shape (M = 25 088, N = 768, K = 192): fv_gemm_bf16 (gemm_nt, the 160 x 128 tiles) against
fv_gemm_bf16_inproj_pk (64-row tiles, weight streamed in fragment order) with full 64-row tiles and with the rows dealt evenly
(49 x 512), HBM-cold (operand sets rotated past the Infinity Cache), timed with events around graphs of 24 launches; each
figure is the best of 8 replays, printed for REPEATS fresh graphs per form, then the median and the spread (max - min) per form
and the gate: median(new) <= median(plain) - 3 x spread(plain).  The first graph of a process is replayed 30 times untimed.
Every form's C is compared with gemm_nt's bit for bit first.
usage: python tools/probe/inproj_fwd_time.py [sets] [repeats]
PROBE_LIB=<path>: load that build of the library instead (a build without the entry point times the plain form only).
PROBE_NO_CHECK=1: go on when C differs (the phase-probe builds -DTPW_DBG=1 / 2 leave C unwritten or wrong on purpose)."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from fastvim_amd import _lib as L_
if os.environ.get("PROBE_LIB"):
    L_.LIB_PATH = os.environ["PROBE_LIB"]
from fastvim_amd import mixer_ops as M
from fastvim_amd.gemm import gemm_nt

Mrows, N, K = 128 * 196, 768, 192
nset = int(sys.argv[1]) if len(sys.argv) > 1 else 8
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dev = "cuda"
g = torch.Generator(device=dev).manual_seed(0)
A = [torch.randn(Mrows, K, device=dev, generator=g).bfloat16() for _ in range(nset)]
W = [(torch.randn(N, K, device=dev, generator=g) * K ** -0.5).bfloat16() for _ in range(nset)]
C = [torch.empty(Mrows, N, device=dev, dtype=torch.bfloat16) for _ in range(nset)]
have = hasattr(L_.lib()._cdll, "fv_gemm_bf16_inproj_pk")
Wpk = []
if have:
    Wpk = [torch.empty(N * K, device=dev, dtype=torch.bfloat16) for _ in range(nset)]
    M.pack_weight_frags_in(W, Wpk)


def plain(i):
    gemm_nt(A[i], W[i])


def packed(rpt):
    return lambda i: M.in_proj_fwd_pk(A[i], Wpk[i], N, rpt)


forms = [("plain gemm_nt", plain)] + ([("packed, 64 rows", packed(64)), ("packed, rows dealt evenly", packed(-1))] if have else [])
if have:
    ref = gemm_nt(A[0], W[0])
    for rpt in (64, -1):
        got = M.in_proj_fwd_pk(A[0], Wpk[0], N, rpt)
        same = torch.equal(ref.view(torch.int16), got.view(torch.int16))
        print(f"rows_per_tile={rpt}: bit-identical to gemm_nt: {same}", flush=True)
        assert same or os.environ.get("PROBE_NO_CHECK")
warm = [True]


def timeit(fn, reps=8):
    n = 24
    gr = torch.cuda.CUDAGraph()
    fn(0)
    torch.cuda.synchronize()
    with torch.cuda.graph(gr):
        for i in range(n):
            fn(i % nset)
    for _ in range(30 if warm[0] else 1):
        gr.replay()
    torch.cuda.synchronize()
    warm[0] = False
    best = 1e9
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); gr.replay(); e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1000 / n)
    return best


res = {name: [] for name, _ in forms}
for _ in range(repeats):            # the forms alternate: one fresh graph of each per round
    for name, fn in forms:
        res[name].append(timeit(fn))
for name, ts in res.items():
    print(f"{name}: " + " / ".join(f"{t:.2f}" for t in ts) + f" us   median {statistics.median(ts):.2f}  spread {max(ts) - min(ts):.2f}", flush=True)
if have:
    base = res["plain gemm_nt"]
    bar = statistics.median(base) - 3 * (max(base) - min(base))
    for name, ts in list(res.items())[1:]:
        print(f"gate ({name}): median {statistics.median(ts):.2f} us against {bar:.2f} us = plain median - 3 x plain spread: "
              + ("PASS" if statistics.median(ts) <= bar else "FAIL"), flush=True)
