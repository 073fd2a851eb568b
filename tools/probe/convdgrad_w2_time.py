"""fv_mixer_conv_pool_bwd_dgrad_pk (plain second weight) against fv_mixer_conv_pool_bwd_dgrad_pk2 (second weight streamed in
fragment order) at the FastVim-T shape, HBM-cold (operand sets rotated past the Infinity Cache), timed with events around
graphs of 24 launches; each figure is the best of 8 replays, printed for REPEATS fresh graphs.  The first graph of a process is
replayed 30 times untimed first (clocks and caches of a cold process cost the first figure 5 us otherwise).
usage: python tools/probe/convdgrad_w2_time.py [sets] [repeats]
PROBE_LIB=<path>: load that build of the library instead (a build without the _pk2 entry point times the plain form only)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from fastvim_amd import _lib as L_
if os.environ.get("PROBE_LIB"):
    L_.LIB_PATH = os.environ["PROBE_LIB"]
from fastvim_amd import mixer_ops as M

B, rows, cols, d_in, d = 128, 14, 14, 384, 192
Mrows, rps = B * rows * cols, rows * cols
nset = int(sys.argv[1]) if len(sys.argv) > 1 else 6
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dev = "cuda"
g = torch.Generator(device=dev).manual_seed(0)
rn = lambda *s: torch.randn(*s, device=dev, generator=g)
sets = []
for _ in range(nset):
    sets.append(dict(xz=rn(B, rps, 2 * d_in).bfloat16(), d_o=rn(B, rps, d_in).bfloat16(), dxc=rn(2, B, rows, d_in),
                     dxc2=rn(2, B, rows, d_in).bfloat16(), dxz=rn(B, rps, 2 * d_in).bfloat16(), gg=rn(Mrows, d), r=rn(Mrows, d),
                     rstd=0.5 + torch.rand(Mrows, device=dev, generator=g)))
cw, cb, cwb, cbb = 0.5 * rn(d_in, 4), 0.1 * rn(d_in), 0.5 * rn(d_in, 4), 0.1 * rn(d_in)
D, Db = 1 + 0.1 * rn(d_in), 1 + 0.1 * rn(d_in)
W_in_t = (rn(2 * d_in, d) * d ** -0.5).bfloat16().t().contiguous()
W_out = (rn(d, d_in) * d_in ** -0.5).bfloat16()
nw = 1 + 0.1 * rn(d)
sc = torch.ones(B, device=dev)
W_in_pk = torch.empty(d * 2 * d_in, device=dev, dtype=torch.bfloat16)
M.pack_weight_frags([W_in_t], [W_in_pk])
have_pk2 = hasattr(L_.lib()._cdll, "fv_mixer_conv_pool_bwd_dgrad_pk2")
W2_pk = None
if have_pk2:
    W2_pk = torch.empty(d * d_in, device=dev, dtype=torch.bfloat16)
    M.pack_weight_frags_w2([W_out], [W2_pk])


def fused(s, tr, w2pk):
    kw = dict(W2_pk=w2pk) if have_pk2 else {}
    M.conv_pool_bwd_dgrad(s["xz"], s["d_o"], s["dxc"], s["dxc2"], cw, cb, cwb, cbb, D, Db, s["dxz"], rows, cols, tr, 1.0, W_in_t,
                          s["gg"], s["r"], s["rstd"], nw, sc, rps, W2=W_out, W_in_pk=W_in_pk, **kw)


warm = [True]


def timeit(tr, w2pk, reps=8):
    n = 24
    gr = torch.cuda.CUDAGraph()
    fused(sets[0], tr, w2pk)
    torch.cuda.synchronize()
    with torch.cuda.graph(gr):
        for i in range(n):
            fused(sets[i % nset], tr, w2pk)
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


for tr in (True, False):
    forms = [("W2 plain", None)] + ([("W2 packed", W2_pk)] if have_pk2 else [])
    for name, w in forms:
        ts = [timeit(tr, w) for _ in range(repeats)]
        print(f"transposed={tr} {name}: " + " / ".join(f"{t:.2f}" for t in ts) + " us", flush=True)
