"""The bf16 GEMM launches of csrc/gemm_mfma.hip, plan by plan: ``fv_gemm_bf16`` and ``fv_gemm_bf16_tn_grouped_ld`` launched
through the C ABI (``fastvim_amd._lib.lib()``) into buffers of the test's own, every output element against its own float64
bound (``gemm_ref.py`` derives the bounds; nothing is measured from the kernels).

Before a launch the test asserts, through the plan query with ``cus = 0`` (this device), that the launch is the kernel the
case means: ``gemm_ref.gemm_cases`` generates the cases for this device's CU count and states each one's key.

Every launch runs twice into freshly allocated outputs prefilled with -16384 (exact in bf16), one tile longer than needed
and, in the strided variants, 8 columns wider (``ldc = N + 8``): the two runs must be bit-identical, no sentinel may be left
where the kernel must write, the slack behind the matrix and the ``ldc - N`` columns between rows must still hold it.  The
padding of padded operand rows (and the other half of the buffer A is a column half of) holds 1000.0.

The float64 products are computed on the GPU by ``torch.matmul`` in float64, over every row: no case reaches the 2e10
multiply-adds from which a row sample (``gemm_ref.sample_rows``) would be allowed, so none samples.

Bit-for-bit relations, each asserted only after the plan query says the two sides are different kernels: a streaming, phased,
eight-wave or 160 x 128 result equals the same product in 2048-row blocks (which run 128 x 96 / 128 x 192 / 128 x 128);
bf16 C equals ``bfloat16(fp32 C)``; a grouped problem equals ``fv_gemm_bf16(a_k_slow = b_k_slow = 1)`` at its split factor;
the in-place form equals partials + ``fv_reduce_partials`` on a gradient that already holds values.

Worst err / bound ratios seen on an MI355X are recorded in DESIGN.md section 4; they are records, not thresholds.
"""
import ctypes

import pytest
import torch

import gemm_ref as R

pytestmark = pytest.mark.gpu

F64, BF16, F32 = torch.float64, torch.bfloat16, torch.float32
SENT = -16384.0
WORST = {}


def _collect():
    """The cases' names, at collection and without touching a GPU: those of a part with 256 CUs (the shapes behind the
    names are generated again for THIS device's CU count by the ``cases`` fixture)."""
    import fastvim_amd.build as fb
    fb.build()
    return [(c["key"][0], c["name"]) for c in R.gemm_cases(256)], R.grouped_cases()


GEMM_NAMES, GROUPED_CASES = _collect()


@pytest.fixture(scope="module")
def lib():
    from fastvim_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def cases(lib):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return {c["name"]: c for c in R.gemm_cases(cus)}


def _L():
    from fastvim_amd import _lib
    return _lib


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def c_long(v):
    return ctypes.c_long(int(v))


def _addr(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def record(kind, r):
    WORST[kind] = max(WORST.get(kind, 0.0), r)


# ----------------------------------------------------------------------------------------------------- fv_gemm_bf16
class Stored:
    """The operands of a case as the launch reads them: padded rows and A's other column half hold R.PAD."""

    def __init__(self, c, A, B, bias):
        M, K, N = c["M"], c["K"], c["N"]
        if c["a_ks"]:
            self.lda, self.offA = M + c["a_pad"], 0
            buf = torch.full((K, self.lda), R.PAD, dtype=BF16)
            buf[:, :M] = A.t()
        elif c["a_half"]:
            self.lda, self.offA = 2 * K, K
            buf = torch.full((M, 2 * K), R.PAD, dtype=BF16)
            buf[:, K:] = A
        else:
            self.lda, self.offA = K, 0
            buf = A.contiguous()
        self.A = buf.cuda()
        if c["b_ks"]:
            self.ldb = N + c["b_pad"]
            buf = torch.full((K, self.ldb), R.PAD, dtype=BF16)
            buf[:, :N] = B
        else:
            self.ldb = K + c["b_pad"]
            buf = torch.full((N, self.ldb), R.PAD, dtype=BF16)
            buf[:, :K] = B.t()
        self.B = buf.cuda()
        self.bias = None if bias is None else bias.cuda()


def launch_gemm(lib, c, s, tile_m, c_fp32=None, row0=0, rows=None):
    """One fv_gemm_bf16 launch of rows [row0, row0 + rows) of the case into a fresh sentinel buffer.  Returns
    (matrix view (splits, rows, ldc), slack, flat buffer)."""
    L = _L()
    M = c["M"] if rows is None else rows
    c_fp32 = c["c_fp32"] if c_fp32 is None else c_fp32
    N, ldc, sp = c["N"], c["N"] + c["ldc_pad"], c["splits"]
    n = sp * M * ldc
    flat = torch.full((n + tile_m * ldc,), SENT, device="cuda", dtype=F32 if c_fp32 else BF16)
    assert row0 == 0 or not c["a_ks"]
    rc = lib.fv_gemm_bf16(_addr(s.A, s.offA + row0 * s.lda), _addr(s.B), _addr(flat), L.ptr(s.bias), L.i32(M), L.i32(N),
                          L.i32(c["K"]), c_long(s.lda), c_long(s.ldb), c_long(ldc), L.i32(c["a_ks"]), L.i32(c["b_ks"]),
                          L.i32(c_fp32), L.i32(sp), L.stream_of(flat))
    L.check(rc, "fv_gemm_bf16")
    return flat[:n].view(sp, M, ldc), flat[n:], flat


def twice(launch, N):
    """Run ``launch`` twice: bit-identical runs, no sentinel left in the matrix, pad columns and slack intact.  Returns
    the first run's (splits, M, N) matrix."""
    (va, sa, fa), (vb, sb, fb) = launch(), launch()
    torch.cuda.synchronize()
    assert torch.equal(_bits(fa), _bits(fb)), "two launches differ"
    for v, s in ((va, sa), (vb, sb)):
        assert bool((s == SENT).all()), "written past the end of the matrix"
        assert bool((v[..., N:] == SENT).all()), "written between the rows (columns N .. ldc)"
        assert not bool((v[..., :N] == SENT).any()), "an element was left unwritten"
    return va[..., :N]


def check_slices(c, C, A, B, bias, first=None):
    """Every K slice of C (splits, M, N) against its own float64 bound, over every row (a row sample only from
    R.SAMPLE_FROM multiply-adds on).  Returns the worst err / bound ratio."""
    rows = None
    if R.macs(c) > R.SAMPLE_FROM:
        rows = R.sample_rows(c["M"], c["tile"][0], c["M"] + c["N"]).cuda()
    A64, B64 = A.cuda().double(), B.cuda().double()
    if rows is not None:
        A64 = A64[rows]
    b64 = None if bias is None else bias.cuda().double()
    if first is not None:
        b64 = first.double() if rows is None else first.double()[rows]
    worst = 0.0
    for s, (k0, k1) in enumerate(R.slices(c["K"], c["splits"])):
        P, S = R.reference(A64, B64, k0, k1)
        target, bnd = R.bound(P, S, k1 - k0, c["c_fp32"], b64)
        got = C[s] if rows is None else C[s][rows]
        r = R.ratio(got, target, bnd)
        worst = max(worst, r.max().item())
        assert worst <= 1.0, f"{c['name']}: slice {s}: {int((r > 1).sum())} elements outside their bound, worst {worst:.3f} x " \
                             f"at {divmod(int(r.argmax()), c['N'])}"
    return worst


@pytest.mark.parametrize("kind,name", GEMM_NAMES, ids=[f"{k}-{n}" for k, n in GEMM_NAMES])
def test_gemm_plan(lib, cases, kind, name):
    assert name in cases, f"no shape reaches the case {name} ({kind}) at this device's CU count"
    c = dict(cases[name])
    assert c["key"][0] == kind
    # the kernel this case means, asserted on THIS device before anything runs
    ldc = c["N"] + c["ldc_pad"]
    p = R.plan(c["M"], c["N"], c["K"], c["a_ks"], c["b_ks"], c["c_fp32"], c["bias"], ldc, c["splits"], 0)
    assert p is not None and (p[0], c["a_ks"], c["b_ks"], c["c_fp32"], p[3]) == c["key"], (p, c["key"])
    c["tile"] = (p[1], p[2])
    A, B, bias = R.operands(c, 7 * c["M"] + 3 * c["N"] + c["K"])
    s = Stored(c, A, B, bias)
    C = twice(lambda: launch_gemm(lib, c, s, p[1]), c["N"])
    worst = check_slices(c, C, A, B, bias)
    record("fp32" if c["c_fp32"] else "bf16", worst)
    rel = []
    # the same product in row blocks that run a different kernel
    if c["blocks"]:
        for r0 in (0, c["M"] - c["blocks"]):
            q = R.plan(c["blocks"], c["N"], c["K"], c["a_ks"], c["b_ks"], c["c_fp32"], c["bias"], ldc, c["splits"], 0)
            assert q is not None and q[0] != p[0], (q, p)
            blk = twice(lambda: launch_gemm(lib, c, s, q[1], row0=r0, rows=c["blocks"]), c["N"])
            assert torch.equal(_bits(blk), _bits(C[:, r0:r0 + c["blocks"]])), f"rows from {r0}: {p[0]} differs from {q[0]}"
            rel.append(f"rows {r0}+ == {q[0]}")
    # bf16 C == bfloat16(fp32 C) where the fp32 output runs another kernel
    if not c["c_fp32"]:
        q = R.plan(c["M"], c["N"], c["K"], c["a_ks"], c["b_ks"], 1, c["bias"], ldc, 1, 0)
        if q is not None and (q[0], q[3]) != (p[0], p[3]):
            c32 = twice(lambda: launch_gemm(lib, c, s, q[1], c_fp32=1), c["N"])
            assert torch.equal(_bits(c32.bfloat16()), _bits(C)), f"bf16 C of {p[0]} differs from bfloat16(fp32 C of {q[0]})"
            rel.append(f"== bfloat16(fp32 C of {q[0]})")
    print(f"{c['name']}: key {c['key']} tile {c['tile']} M {c['M']} N {c['N']} K {c['K']} splits {c['splits']}: "
          f"err / bound {worst:.4f}; {'; '.join(rel)}")
    print("worst so far", {k: round(v, 4) for k, v in sorted(WORST.items())})


# -------------------------------------------------------------------------------------------- grouped weight gradients
def _arr(ty, vals):
    return (ty * len(vals))(*vals)


class Group:
    """Operands of a grouped call on the device (x (Kd, ldx), y (Kd, ldy), padding = R.PAD) and, for the in-place
    problems, the gradient the product is added to."""

    def __init__(self, problems, seed):
        g = torch.Generator().manual_seed(seed)
        self.problems, self.x, self.y, self.X, self.Y, self.first = problems, [], [], [], [], []
        for q in problems:
            X = torch.randn(q["Kd"], q["M"], generator=g).bfloat16()
            Y = torch.randn(q["Kd"], q["N"], generator=g).bfloat16()
            xb = torch.full((q["Kd"], q["ldx"]), R.PAD, dtype=BF16)
            xb[:, :q["M"]] = X
            yb = torch.full((q["Kd"], q["ldy"]), R.PAD, dtype=BF16)
            yb[:, :q["N"]] = Y
            self.X.append(X), self.Y.append(Y), self.x.append(xb.cuda()), self.y.append(yb.cuda())
            self.first.append(torch.randn(q["M"], q["N"], generator=g).cuda() if q["splits"] == -1 else None)

    def outputs(self):
        """Fresh outputs: (splits, M, N) partials (the gradient itself for an in-place problem) + 256 rows of slack."""
        flats = []
        for q, f in zip(self.problems, self.first):
            n = max(q["splits"], 1) * q["M"] * q["N"]
            flat = torch.full((n + 256 * q["N"],), SENT, device="cuda", dtype=F32)
            if f is not None:
                flat[:n] = f.reshape(-1)
            flats.append(flat)
        return flats

    def launch(self, lib, splits=None):
        L = _L()
        P, I = ctypes.c_void_p, ctypes.c_int
        ps = self.problems
        flats = self.outputs()
        rc = lib.fv_gemm_bf16_tn_grouped_ld(_arr(P, [t.data_ptr() for t in self.x]), _arr(P, [t.data_ptr() for t in self.y]),
                                            _arr(P, [t.data_ptr() for t in flats]), _arr(I, [q["Kd"] for q in ps]),
                                            _arr(I, [q["M"] for q in ps]), _arr(I, [q["N"] for q in ps]),
                                            _arr(I, [q["ldx"] for q in ps]), _arr(I, [q["ldy"] for q in ps]),
                                            _arr(I, splits or [q["splits"] for q in ps]), L.i32(len(ps)), L.stream_of(flats[0]))
        return rc, flats


def _single(lib, q, x, y):
    """The problem through fv_gemm_bf16(a_k_slow = b_k_slow = 1) at its split factor; extents rounded up to 8 where the
    grouped entry takes them through ldx / ldy (the extra rows and columns multiply padding and are cut off)."""
    L = _L()
    Mr, Nr, sp = (q["M"] + 7) // 8 * 8, (q["N"] + 7) // 8 * 8, max(q["splits"], 1)
    out = torch.full((sp, Mr, Nr), SENT, device="cuda", dtype=F32)
    rc = lib.fv_gemm_bf16(_addr(x), _addr(y), _addr(out), None, L.i32(Mr), L.i32(Nr), L.i32(q["Kd"]), c_long(q["ldx"]),
                          c_long(q["ldy"]), c_long(Nr), L.i32(1), L.i32(1), L.i32(1), L.i32(sp), L.stream_of(out))
    L.check(rc, "fv_gemm_bf16")
    return out[:, :q["M"], :q["N"]]


@pytest.mark.parametrize("g", GROUPED_CASES, ids=[g["name"] for g in GROUPED_CASES])
def test_grouped_plan(lib, g):
    L = _L()
    ps = g["problems"]
    keys = [R.grouped_plan(l) for l in R.grouped_launches(ps)]
    assert keys == g["keys"], (keys, g["keys"])
    G = Group(ps, len(ps) + ps[0]["Kd"])
    (rca, fa), (rcb, fb) = G.launch(lib), G.launch(lib)
    L.check(rca, "fv_gemm_bf16_tn_grouped_ld"), L.check(rcb, "fv_gemm_bf16_tn_grouped_ld")
    torch.cuda.synchronize()
    worst, rel = 0.0, set()
    launch_of = [k for l, k in zip(R.grouped_launches(ps), keys) for _ in l]
    for i, (q, a, b) in enumerate(zip(ps, fa, fb)):
        sp = max(q["splits"], 1)
        n = sp * q["M"] * q["N"]
        assert torch.equal(_bits(a), _bits(b)), f"problem {i}: two launches differ"
        assert bool((a[n:] == SENT).all()) and bool((b[n:] == SENT).all()), f"problem {i}: written past its end"
        assert not bool((a[:n] == SENT).any()), f"problem {i}: an element was left unwritten"
        C = a[:n].view(sp, q["M"], q["N"])
        c = dict(name=f"{g['name']}[{i}]", M=q["M"], N=q["N"], K=q["Kd"], c_fp32=1, splits=sp, tile=R.GROUPED_TILES[launch_of[i][0]])
        worst = max(worst, check_slices(c, C, G.X[i].t(), G.Y[i], None, first=G.first[i]))
        if q["splits"] != -1:
            # the grouped kernel against the single launch (another kernel: 128 x 128 tiles, its own tile walk)
            assert R.plan((q["M"] + 7) // 8 * 8, (q["N"] + 7) // 8 * 8, q["Kd"], 1, 1, 1, 0, (q["N"] + 7) // 8 * 8, sp, 0)[0] == "128x128"
            assert torch.equal(_bits(C), _bits(_single(lib, q, G.x[i], G.y[i]))), f"problem {i} differs from fv_gemm_bf16"
            rel.add("== fv_gemm_bf16(a_k_slow = b_k_slow = 1)")
    if any(q["splits"] == -1 for q in ps):
        # in place == one partial + fv_reduce_partials (accumulate) on the same gradient.  (The partial route of these
        # outputs is the same phased kernel with the storing epilogue: the plan query has no second kernel to confirm.)
        sp1 = [1 if q["splits"] == -1 else q["splits"] for q in ps]
        assert keys[0][2] == 1 and R.grouped_plan([dict(q, splits=s) for q, s in zip(ps, sp1)]) == keys[0]
        # the partials go into sentinel buffers that do not hold the gradient
        firsts, G.first = G.first, [None] * len(ps)
        try:
            rc, parts = G.launch(lib, splits=sp1)
        finally:
            G.first = firsts
        L.check(rc, "fv_gemm_bf16_tn_grouped_ld")
        for q, a, part, f in zip(ps, fa, parts, firsts):
            if f is None:
                continue
            n = q["M"] * q["N"]
            out = f.clone()
            rc = lib.fv_reduce_partials(_addr(part), _addr(out), L.i32(1), ctypes.c_size_t(n), L.i32(1), L.stream_of(out))
            L.check(rc, "fv_reduce_partials")
            assert torch.equal(_bits(a[:n]), _bits(out.reshape(-1))), "in place differs from partials + fv_reduce_partials"
        rel.add("in place == partials + fv_reduce_partials")
    record("grouped fp32", worst)
    print(f"{g['name']}: keys (tile class, lds_dma, phased) {keys}, {len(ps)} problems: err / bound {worst:.4f}; {'; '.join(sorted(rel))}")
    print("worst so far", {k: round(v, 4) for k, v in sorted(WORST.items())})


def test_grouped_refusals(lib):
    """What the grouped entry documents it refuses: the plan query and the entry agree, and nothing is written."""
    for ps in R.GROUPED_REFUSED:
        assert R.grouped_plan(ps) is None
        G = Group(ps, 5)
        rc, flats = G.launch(lib)
        torch.cuda.synchronize()
        assert rc != 0
        for q, f, first in zip(ps, flats, G.first):
            n = q["M"] * q["N"]
            assert bool((f[n:] == SENT).all())
            assert torch.equal(f[:n], first.reshape(-1)) if first is not None else bool((f[:n] == SENT).all())
