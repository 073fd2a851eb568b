"""The channel-last scan launches of csrc/scan_cl.hip, each on its own against the float64 reference of
``scan_cl_ref.py``, launch key by launch key: ``fv_mixer_scan_fwd_seg``, ``fv_mixer_xproj_scan_fwd``,
``fv_mixer_scan_bwd_seg`` and ``fv_mixer_scan_bwd_xproj`` through the C ABI into the test's own buffers.

A launch's KEY is what selects its code; all of it is read from queries the library exports plus ``(Lc, dt_rank)``:

forward   ("fused", rank class, LCC, exact, channel chunks 1 / 2 / 3+)      fv_mixer_xproj_scan_fwd_ok (bf16 only)
          ("chunked", dtype, rank class, segments?, checkpoints wanted?)     Lc > 16 and dt_rank <= 48; fv_mixer_scan_fwd_segments
          ("generic", dtype, rank class)                                     everything else
backward  ("short" | "fold", dtype, rank class, LCC, exact, NBB)             Lc <= 16 and dt_rank <= 48; fv_mixer_scan_bwd_xproj_ok;
                                                                             NBB = batch / fv_mixer_scan_bwd_partials
          ("chunked", dtype, rank class, waves 4 | 12, checkpoints given?)   fv_mixer_scan_bwd_chunks_b
          ("chunked_seg", dtype, rank class)                                 given checkpoints + workspace, fv_mixer_scan_bwd_segments > 1
          ("generic", dtype, rank class, checkpoints in "lds" | "global")    fv_mixer_scan_bwd_ckpt_floats == 0 or not

rank class: ceil(dt_rank / 4) in <= 3 / <= 6 / <= 12 / <= 24 (the RQ template argument); LCC / exact: the short kernels are
built for 14 and 16 rows, exact when Lc is 14 or 16, else the next one up with a bound check per step.

CASES is generated key by key: every case STATES the keys its launches are there for, computed from the attributes it
was generated from, and every test first asserts through the library's queries that its shape still has them.
``test_scan_cl_ref_cpu.py`` sweeps the queries and asserts that every key reachable with the default settings occurs
here.  Left out, and why: the generic backward's rank classes <= 3 / 6 / 12 (dt_rank <= 48 reaches the generic backward
only through the FASTVIM_* tuning variables, which nothing here sets); the folded kernel at NBB 4 / 8 (it is fixed at
d_inner 384, where those need a batch of 512 or more: NBB 4 / 8 are covered on the unfolded kernel, same code path).

Every launch runs twice into fresh buffers that are prefilled with a sentinel and one row (or one slice) longer than the
library's size queries say: the two runs must be bit-identical (no atomics), nothing may be left unwritten except the
slots a kernel leaves alone by design (the first chunk's checkpoint: the zero state no kernel stores), and the slack
must still hold the sentinel.

What is compared, and the bounds (``scan_cl_ref.TOL_*``: the project's fp32 ones, none fitted to the kernels), each times
``max(1, max|ref|)`` of the PIECE compared: y and du 1e-5 / 2e-5 per (direction, batch element); the forward's
checkpoints 1e-5 per (direction, element), every chunk; every dx_dbl channel-chunk slice on its own 5e-5; every
parameter-gradient partial row on its own 1e-4 (segment-parallel: the sum of an element's rows).  Inputs are rounded to
the storage dtype before the reference sees them, so bf16 launches keep the same bounds.  The fused forward's bf16 x_dbl
is held per element to ``2**-8 |P64| + d_in 2**-24 (|xc| @ |Wx|^T)`` and its y to the reference evaluated on the x_dbl
the kernel stored.  The folded backward's ``dxc + dxc2`` is held to du + dx_dbl @ Wx: fp32 at the du bound; bf16 storage
adds the rounding of its bf16 matrix-core product and of the bf16 ``dxc2`` (test_xproj_fold_gpu.py's derivation).
"""
import ctypes

import pytest
import torch

import scan_cl_ref as S

N = S.N
DTS = ("f32", "bf16")
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
cdiv = lambda a, b: -(-a // b)


# ------------------------------------------------------------------------------------------------ keys (host only)
def rank_class(R):
    rq = cdiv(R, 4)
    return 3 if rq <= 3 else 6 if rq <= 6 else 12 if rq <= 12 else 24


def lcc_exact(Lc):
    return (14, Lc == 14) if Lc <= 14 else (16, Lc == 16)


class Queries:
    def __init__(self, lib):
        self.lib = lib

    def _q(self, name, *a):
        return getattr(self.lib, name)(*[ctypes.c_int(int(v)) for v in a])

    def fused_ok(self, Lc, d, R, dt):
        return bool(self._q("fv_mixer_xproj_scan_fwd_ok", Lc, d, R, DTS.index(dt)))

    def fold_ok(self, B, Lc, d, R, dt):
        return bool(self._q("fv_mixer_scan_bwd_xproj_ok", B, Lc, d, R, DTS.index(dt)))

    def segments(self, B, Lc, d, R):
        s = self._q("fv_mixer_scan_fwd_segments", B, Lc, d, R)
        assert s == self._q("fv_mixer_scan_bwd_segments", B, Lc, d, R)
        return s

    def nbb(self, B, Lc, R):
        rows = self._q("fv_mixer_scan_bwd_partials", B, Lc, R)
        assert B % rows == 0
        return B // rows

    def bwd_waves(self, B, Lc, d, R):
        """Waves of the chunked backward's workgroups: the rule depends on cdiv(d_inner, 192) and the batch only, and at a
        multiple of 192 channels the two widths give different chunk counts."""
        d192 = 192 * cdiv(d, 192)
        n = self._q("fv_mixer_scan_bwd_chunks_b", B, d192, Lc, R)
        assert n in (d192 // 192, d192 // 64)
        return 12 if n == d192 // 192 else 4

    def fwd_ckpt_floats(self, B, Lc, d, R):
        return self._q("fv_mixer_scan_ckpt_floats", B, Lc, d, N, R)

    def bwd_ckpt_floats(self, B, Lc, d, R):
        return self._q("fv_mixer_scan_bwd_ckpt_floats", B, Lc, d, N, R)

    def fwd_key(self, B, Lc, d, R, dt, want_ckpt=False, ws=True, fused=None):
        if fused is None:
            fused = dt == "bf16" and self.fused_ok(Lc, d, R, dt)
        if fused:
            return ("fused", rank_class(R)) + lcc_exact(Lc) + (min(cdiv(d, 192), 3),)
        if Lc > 16 and R <= 48:
            return ("chunked", dt, rank_class(R), ws and self.segments(B, Lc, d, R) > 1, want_ckpt)
        return ("generic", dt, rank_class(R))

    def bwd_key(self, B, Lc, d, R, dt, given=False, ws=True, fold=False):
        if Lc <= 16 and R <= 48:
            return ("fold" if fold else "short", dt, rank_class(R)) + lcc_exact(Lc) + (self.nbb(B, Lc, R),)
        assert self.nbb(B, Lc, R) == 1
        if R <= 48:
            if given and ws and self.segments(B, Lc, d, R) > 1:
                return ("chunked_seg", dt, rank_class(R))
            return ("chunked", dt, rank_class(R), self.bwd_waves(B, Lc, d, R), given)
        return ("generic", dt, rank_class(R), "lds" if self.bwd_ckpt_floats(B, Lc, d, R) == 0 else "global")


# keys the sweep reaches that have no case here (module docstring)
LEFT_OUT = {("fold", dt, 3, lc, True, nbb) for dt in DTS for lc in (14, 16) for nbb in (4, 8)}


# ------------------------------------------------------------------------------------------------ the case table
R_OF = {3: (1, 2, 7, 12), 6: (13, 24), 12: (25, 48)}       # dt_rank per rank class: both ends of a class, odd ranks
D_SMALL = (40, 64, 72, 200)                                 # lanes / whole waves past the row, a last channel chunk of 8
CASES = []


def _add(kind, B, Lc, d, R, dt, fwd=(), bwd=(), dpd=False, **kw):
    name = f"{kind}_b{B}_l{Lc}_d{d}_r{R}_{dt}" + ("_dpd" if dpd else "")
    CASES.append(dict(name=name, kind=kind, B=B, Lc=Lc, d=d, R=R, dt=dt, fwd=tuple(fwd), bwd=tuple(bwd), dpd=dpd,
                      seed=5000 + len(CASES), **kw))


def _short_cases():
    # j counts the (dtype, rank class, LCC, exact) combinations; every choice below is indexed by j (shifted per rank class,
    # since j % 4 alone is the LCC / exact index) and by the NBB index, never by a counter that the innermost loop advances.
    # Every combination has a row wider than one 192-channel workgroup with a tail chunk (200: 192 + 8; 392: 2 x 192 + 8) at
    # NBB 1 or 2 -- second and third workgroups, their dx_dbl slices and partial-row columns -- and the generic forward
    # that rides on these shapes gets 2 to 7 blocks of 64 channels
    D_NBB1, D_NBB2 = (200, 72, 392, 40), (64, 200, 40, 200)
    j = 0
    for dt in DTS:
        for rc in (3, 6, 12):
            for lcc, exact in ((14, True), (14, False), (16, True), (16, False)):
                jj = j + j // 4
                for ni, nbb in enumerate((1, 2, 4, 8)):
                    Lc = lcc if exact else 15 if lcc == 16 else (1, 2, 13)[(jj + ni) % 3]
                    if nbb <= 2:
                        R, B = R_OF[rc][(jj + ni) % len(R_OF[rc])], 3 if nbb == 1 else 2
                        d = (D_NBB1 if nbb == 1 else D_NBB2)[jj % 4]
                    else:
                        # NBB depends on (batch, Lc, dt_rank) only: the largest rank of the class (most channel chunks of
                        # a 32 dt_rank wide model, smallest batch), on a narrow row -- two workgroups wide at batch 128 / 132
                        R = R_OF[rc][-1]
                        chunks = cdiv(32 * R, 192)
                        B = 8 * cdiv(128, chunks) if nbb == 8 else 4 * cdiv(256, chunks) + 4
                        d = (64, 200)[j % 2] if rc == 12 else 24
                    # the product runs the generic forward at these lengths wherever the fused launch does not take the
                    # shape (fp32; bf16 with d_inner no multiple of 32)
                    fwd = [("generic", dt, rc)] if dt == "f32" or d % 32 else []
                    _add("short", B, Lc, d, R, dt, fwd=fwd, bwd=[("short", dt, rc, lcc, exact, nbb)], dpd=(j == 0 and nbb == 2), nbb=nbb)
                j += 1


def _chunked_cases():
    twelve = {("f32", 3): (128, 17, 64, 2), ("bf16", 3): (128, 33, 200, 6), ("f32", 6): (64, 37, 200, 13),
              ("bf16", 6): (128, 32, 40, 24), ("f32", 12): (64, 17, 200, 25), ("bf16", 12): (128, 33, 72, 48)}
    k = 0               # counts (dtype, rank class): the four-wave choices are indexed by it, not by the waves loop
    for dt in DTS:
        for rc in (3, 6, 12):
            for waves in (4, 12):
                if waves == 4:      # Lc: a second chunk of one step, exact chunks, ragged chunks
                    B, Lc, d, R = 2 + k % 2, (17, 32, 33, 37)[k % 4], D_SMALL[(k + 1) % 4], R_OF[rc][(k // 3 + 2) % len(R_OF[rc])]
                else:
                    B, Lc, d, R = twelve[dt, rc]
                _add("chunked", B, Lc, d, R, dt, fwd=[("chunked", dt, rc, False, w) for w in (False, True)],
                     bwd=[("chunked", dt, rc, waves, g) for g in (False, True)], dpd=(k == 1 and waves == 12), nbb=1)
            k += 1
    # segment-parallel: Lc >= 241 on few workgroups.  (1, 241, 64, .): 2 segments and a last chunk of one step;
    # (1, 400, 72, .): 3 segments of 9, 9 and 7 chunks.  Each also runs without the workspace pointer (serial).  Two of
    # the 241-step cases have batch 2 (still 2 segments): the partial rows are (element, segment) ordered, which one
    # element cannot tell from (segment, element)
    for j, (dt, rc) in enumerate((dt, rc) for dt in DTS for rc in (3, 6, 12)):
        B, Lc, d, segs = ((1, 241, 64, 2), (1, 400, 72, 3), (2, 241, 64, 2), (1, 400, 72, 3), (2, 241, 64, 2), (1, 400, 72, 3))[j]
        R = {3: (2, 6), 6: (13, 24), 12: (25, 48)}[rc][j % 2]
        _add("seg", B, Lc, d, R, dt, fwd=[("chunked", dt, rc, s, w) for s in (False, True) for w in (False, True)],
             bwd=[("chunked_seg", dt, rc), ("chunked", dt, rc, 4, True)], dpd=(j == 0), nbb=1, segs=segs)


def _generic_cases():
    # dt_rank > 48: FastVim-L / -H (64, 80) at 14 rows; the last Lc with the checkpoints in LDS and the first with them in
    # global scratch, at a partial last rank quad; dt_rank 96 at the forward's LDS limit
    for dt in DTS:
        for B, Lc, d, R, ck in ((2, 14, 72, 64, "lds"), (2, 14, 64, 80, "lds"), (2, 24, 64, 49, "lds"), (2, 25, 64, 49, "global"),
                                (1, 128, 64, 96, "global")):
            _add("generic", B, Lc, d, R, dt, fwd=[("generic", dt, 24)], bwd=[("generic", dt, 24, ck)],
                 dpd=(dt, Lc) in (("f32", 24), ("bf16", 25)), nbb=1)


def _fused_cases():
    d_of = {1: (32, 64), 2: (224, 384), 3: (416, 576, 768)}
    i = 0
    for rc in (3, 6, 12):
        for lcc, exact in ((14, True), (14, False), (16, True), (16, False)):
            for nch in (1, 2, 3):
                Lc = lcc if exact else 15 if lcc == 16 else (1, 9)[i % 2]
                _add("fused", 2 + i % 2, Lc, d_of[nch][(i // 3) % len(d_of[nch])], R_OF[rc][i % len(R_OF[rc])], "bf16",
                     fwd=[("fused", rc, lcc, exact, nch)])
                i += 1


def _fold_cases():
    i = 0
    for dt in DTS:
        for Lc in (14, 16):
            for nbb in (1, 2):
                _add("fold", 3 if nbb == 1 else (2, 4)[(i // 2) % 2], Lc, 384, (2, 7, 12)[i % 3], dt, bwd=[("fold", dt, 3, Lc, True, nbb)], nbb=nbb)
                i += 1


_short_cases()
_chunked_cases()
_generic_cases()
_fused_cases()
_fold_cases()
CASE_BY_NAME = {c["name"]: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


def names(*kinds):
    return [c["name"] for c in CASES if c["kind"] in kinds]


def make_inputs(c):
    return S.make_inputs(c["B"], c["Lc"], c["d"], c["R"], c["dt"] == "bf16", c["seed"], dyc_per_direction=c["dpd"],
                         with_wx=c["kind"] in ("fused", "fold"))


def bwd_chunk_channels(c, segmented=False):
    """Channels per dx_dbl slice of a case's backward launch."""
    if c["kind"] in ("short", "fold"):
        return 192
    if c["kind"] in ("generic", "seg") or segmented:      # (the segment cases' serial launches: 4 waves)
        return 64
    return 16 * c["bwd"][0][3]


def assert_keys(q, c):
    """The keys a case states are the keys the library's queries give its shape."""
    a = (c["B"], c["Lc"], c["d"], c["R"], c["dt"])
    if c["kind"] == "fused":
        assert q.fused_ok(*a[1:]) and [q.fwd_key(*a)] == list(c["fwd"]), (c["name"], q.fwd_key(*a))
        return
    if c["fwd"]:
        got = sorted({q.fwd_key(*a, want_ckpt=w, ws=s, fused=False) for w in (False, True) for s in (False, True)}, key=str)
        assert got == sorted(c["fwd"], key=str), (c["name"], got)
        assert not (c["dt"] == "bf16" and q.fused_ok(*a[1:])), "the product runs the fused launch at this shape"
    fold = c["kind"] == "fold"
    assert not fold or q.fold_ok(*a)
    got = sorted({q.bwd_key(*a, given=g, ws=s, fold=fold) for g in ((False, True) if c["Lc"] > 16 and c["R"] <= 48 else (False,))
                  for s in (False, True)}, key=str)
    want = set(c["bwd"]) | ({("chunked", c["dt"], rank_class(c["R"]), 4, False)} if c["kind"] == "seg" else set())
    assert got == sorted(want, key=str), (c["name"], got)
    if "segs" in c:
        assert q.segments(*a[:4]) == c["segs"]


# ------------------------------------------------------------------------------------------------ GPU side
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import fastvim_amd.build as fb
    fb.build()
    from fastvim_amd import _lib
    return _lib.lib()


class Buf:
    """A device buffer of n elements prefilled with the sentinel, with ``slack`` more behind it."""

    def __init__(self, n, slack, dtype=torch.float32):
        self.flat = torch.full((n + slack,), S.SENTINEL, device="cuda", dtype=dtype)
        self.out, self.slack = self.flat[:n], self.flat[n:]

    def intact(self):
        return bool((self.slack == S.SENTINEL).all())

    def unwritten(self):
        return int((self.out == S.SENTINEL).sum())


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _twice(launch):
    """launch() -> (return code, {name: Buf}).  Runs it twice; returns the first run's buffers after asserting the return
    code, bit equality of the two runs and the untouched slack."""
    (rc1, a), (rc2, b) = launch(), launch()
    torch.cuda.synchronize()
    from fastvim_amd import _lib as L
    assert rc1 == 0 and rc2 == 0, L.lib().fv_last_error().decode()
    for k in a:
        assert torch.equal(_bits(a[k].flat), _bits(b[k].flat)), f"{k}: two launches differ"
        assert a[k].intact(), f"{k}: the slack behind the buffer was written"
    return a


class Dev:
    """A case's inputs on the device, in the storage dtype."""

    def __init__(self, c, inp):
        dt = TDT[c["dt"]]
        self.xc, self.x_dbl = inp["xc"].to("cuda", dt), inp["x_dbl"].to("cuda", dt)
        self.par = [inp[k][j].contiguous().cuda() for j in (0, 1) for k in ("Wdt", "bdt", "A_log")]      # dt_w, dt_b, A_log, then _b
        self.dyc = inp["dyc"].contiguous().cuda()
        if "Wx" in inp:
            self.Wx = [inp["Wx"][j].contiguous().cuda() for j in (0, 1)]
            self.Wx2 = inp["Wx"].to("cuda", torch.bfloat16).contiguous()


def _shape_args(c):
    from fastvim_amd import _lib as L
    return [L.i32(c["B"]), L.i32(c["Lc"]), L.i32(c["d"]), L.i32(c["R"]), L.i32(N), L.i32(DTS.index(c["dt"]))]


def launch_fwd(lib, q, c, dev, want_ckpt, ws):
    from fastvim_amd import _lib as L
    B, Lc, d, R = c["B"], c["Lc"], c["d"], c["R"]
    nchunk = cdiv(Lc, 16)
    nck = q.fwd_ckpt_floats(B, Lc, d, R) if want_ckpt else 0
    assert q.fwd_ckpt_floats(B, Lc, d, R) == (2 * B * nchunk * d * N if Lc > 16 and R <= 48 else 0)
    nws = lib.fv_mixer_scan_fwd_seg_floats(*_shape_args(c)[:3], L.i32(N), L.i32(R)) if ws else 0
    if ws:
        segs = q.segments(B, Lc, d, R)
        assert nws == (2 * B * segs * d * (2 * N + 1) if segs > 1 else 0)

    def launch():
        bufs = dict(yc=Buf(2 * B * Lc * d, d))
        if nck:
            bufs["ckpt"] = Buf(nck, d * N)
        if nws:
            bufs["ws"] = Buf(nws, d)
        rc = lib.fv_mixer_scan_fwd_seg(L.ptr(dev.xc), L.ptr(dev.x_dbl), *[L.ptr(t) for t in dev.par], L.ptr(bufs["yc"].flat),
                                       L.ptr(bufs["ckpt"].flat if nck else None), L.ptr(bufs["ws"].flat if nws else None),
                                       *_shape_args(c), L.stream_of(dev.xc))
        return rc, bufs

    return launch


def check_fwd_outputs(c, bufs):
    B, Lc, d = c["B"], c["Lc"], c["d"]
    assert bufs["yc"].unwritten() == 0, "yc has unwritten elements"
    yc = bufs["yc"].out.view(2, B, Lc, d)
    ck = None
    if "ckpt" in bufs:
        # by design the forward kernels store the state entering chunks 1..: the first chunk's slot stays as it was
        ck = bufs["ckpt"].out.view(2, B, cdiv(Lc, 16), d, N)
        assert bool((ck[:, :, 0] == S.SENTINEL).all()), "the first chunk's checkpoint slot was written"
        assert not bool((ck[:, :, 1:] == S.SENTINEL).any()), "a checkpoint of chunks 1.. is unwritten"
    return yc, ck


def launch_bwd(lib, q, c, dev, ckpt, ws):
    """ckpt: the forward launch's checkpoints (given) or None (the kernel sweeps forward itself)."""
    from fastvim_amd import _lib as L
    B, Lc, d, R = c["B"], c["Lc"], c["d"], c["R"]
    W, per_row = R + 2 * N, 2 * d * (N + R + 1)
    given = ckpt is not None
    segs = q.segments(B, Lc, d, R) if (ws and given) else 1
    nws = lib.fv_mixer_scan_bwd_seg_floats(*_shape_args(c)[:3], L.i32(N), L.i32(R)) if (ws and given) else 0
    assert nws == (2 * B * segs * d * (2 * N + 1) if segs > 1 else 0)
    nch = lib.fv_mixer_scan_bwd_seg_chunks(L.i32(B), L.i32(d), L.i32(Lc), L.i32(R), L.i32(int(nws > 0)))
    assert nch == cdiv(d, bwd_chunk_channels(c, segs > 1))
    rows = lib.fv_mixer_scan_bwd_seg_partials(L.i32(B), L.i32(Lc), L.i32(d), L.i32(R)) if nws else B // q.nbb(B, Lc, R)
    assert rows == (B * segs if nws else B // c["nbb"])
    nck = 0 if given else q.bwd_ckpt_floats(B, Lc, d, R)
    kind = c["bwd"][0][0]
    assert nck == (0 if given or kind == "short" or c["bwd"][0][-1] == "lds" else
                   2 * B * cdiv(Lc, 16) * d * N if kind in ("chunked", "chunked_seg") else 2 * B * cdiv(Lc, 4) * d * N)

    def launch():
        bufs = dict(dxc=Buf(2 * B * Lc * d, d), dx_dbl=Buf(nch * 2 * B * Lc * W, 2 * B * Lc * W), part=Buf(rows * per_row, per_row))
        if nck:
            bufs["scratch"] = Buf(nck, d * N)
        if nws:
            bufs["ws"] = Buf(nws, d)
        ck = ckpt if given else bufs["scratch"].flat if nck else None
        rc = lib.fv_mixer_scan_bwd_seg(L.ptr(dev.xc), L.ptr(dev.x_dbl), *[L.ptr(t) for t in dev.par], L.ptr(dev.dyc), L.i32(int(c["dpd"])),
                                       L.ptr(bufs["dxc"].flat), L.ptr(bufs["dx_dbl"].flat), L.ptr(ck), L.i32(int(given)),
                                       L.ptr(bufs["part"].flat), L.ptr(bufs["ws"].flat if nws else None), *_shape_args(c),
                                       L.stream_of(dev.xc))
        return rc, bufs

    return launch, nch, rows, segs


def check_bwd_outputs(c, bufs, nch, rows):
    B, Lc, d, W = c["B"], c["Lc"], c["d"], c["R"] + 2 * N
    for k in ("dxc", "dx_dbl", "part"):
        assert bufs[k].unwritten() == 0, f"{k} has unwritten elements"
    return bufs["dxc"].out.view(2, B, Lc, d), bufs["dx_dbl"].out.view(nch, 2, B * Lc, W), bufs["part"].out.view(rows, -1)


_REFS = {}


def ref_of(name, chunk_channels):
    """The float64 reference of a case, computed once and shared by the tests of the case."""
    key = (name, chunk_channels)
    if key not in _REFS:
        if len(_REFS) >= 3:
            _REFS.pop(next(iter(_REFS)))
        inp = make_inputs(CASE_BY_NAME[name])
        _REFS[key] = (inp, S.reference(inp, chunk_channels=chunk_channels))
    return _REFS[key]


def _report(name, rep):
    print(f"\nratios {name} " + " ".join(f"{k}={v:.3f}" for k, v in sorted(rep.ratios.items())))
    rep.check(name)


@pytest.mark.parametrize("name", [c["name"] for c in CASES if c["kind"] != "fused" and c["fwd"]])
def test_scan_fwd_vs_fp64(lib, name):
    """fv_mixer_scan_fwd_seg: with and without checkpoints, and (segment cases) with and without the workspace."""
    c, q = CASE_BY_NAME[name], Queries(lib)
    assert_keys(q, c)
    inp, ref = ref_of(name, None)          # y and checkpoints only: no chunk slices
    dev, rep = Dev(c, inp), S.Report()
    for ws in ((False, True) if c["kind"] == "seg" else (True,)):
        for want in ((False, True) if c["kind"] in ("chunked", "seg") else (False,)):
            assert q.fwd_key(c["B"], c["Lc"], c["d"], c["R"], c["dt"], want, ws, fused=False) in c["fwd"]
            yc, ck = check_fwd_outputs(c, _twice(launch_fwd(lib, q, c, dev, want, ws)))
            assert (ck is not None) == want
            S.compare_forward(rep, yc, ref, ck)
    _report(name, rep)


@pytest.mark.parametrize("name", names("short", "chunked", "seg", "generic"))
def test_scan_bwd_vs_fp64(lib, name):
    """fv_mixer_scan_bwd_seg: sweeping its own checkpoints and (chunked) with the forward launch's, segment-parallel and
    serial.  The given checkpoints are the forward launch's own, first-chunk sentinel included (the kernel reads that
    slot and must mask it)."""
    c, q = CASE_BY_NAME[name], Queries(lib)
    assert_keys(q, c)
    seg = c["kind"] == "seg"
    dev = rep = None
    for segmented in ((False, True) if seg else (False,)):
        inp, ref = ref_of(name, bwd_chunk_channels(c, segmented))
        dev, rep = dev or Dev(c, inp), rep or S.Report()
        modes = [(True, True)] if segmented else [(False, False), (True, False)] if c["kind"] in ("chunked", "seg") else [(False, False)]
        for given, ws in modes:
            assert q.bwd_key(c["B"], c["Lc"], c["d"], c["R"], c["dt"], given, ws) in set(c["bwd"]) | {("chunked", c["dt"], rank_class(c["R"]), 4, False)}
            ckpt = None
            if given:
                ckpt = _twice(launch_fwd(lib, q, c, dev, True, ws))["ckpt"].flat
            launch, nch, rows, segs = launch_bwd(lib, q, c, dev, ckpt, ws)
            assert (segs > 1) == segmented
            dxc, sl, part = check_bwd_outputs(c, _twice(launch), nch, rows)
            S.compare_backward(rep, dxc, sl, part, ref, nbb=c["nbb"], segments=segs)
    _report(name, rep)


@pytest.mark.parametrize("name", names("fused"))
def test_fused_xproj_scan_fwd_vs_fp64(lib, name):
    from fastvim_amd import _lib as L
    c, q = CASE_BY_NAME[name], Queries(lib)
    assert_keys(q, c)
    B, Lc, d, R = c["B"], c["Lc"], c["d"], c["R"]
    W = R + 2 * N
    inp = make_inputs(c)
    dev = Dev(c, inp)

    def launch():
        bufs = dict(x_dbl=Buf(2 * B * Lc * W, W, torch.bfloat16), yc=Buf(2 * B * Lc * d, d))
        rc = lib.fv_mixer_xproj_scan_fwd(L.ptr(dev.xc), L.ptr(dev.Wx2), *[L.ptr(t) for t in dev.par], L.ptr(bufs["x_dbl"].flat),
                                         L.ptr(bufs["yc"].flat), *_shape_args(c), L.stream_of(dev.xc))
        return rc, bufs

    bufs = _twice(launch)
    assert bufs["x_dbl"].unwritten() == 0 and bufs["yc"].unwritten() == 0
    x_dbl = bufs["x_dbl"].out.view(2, B * Lc, W).float().cpu()
    rep = S.Report()
    P, bound = S.fused_xdbl_ref(inp["xc"], inp["Wx"])
    rep.add_elementwise("x_dbl", x_dbl, P, bound)
    y, _ = S.scan(inp["xc"].double(), x_dbl.double(), inp["Wdt"].double(), inp["bdt"].double(), inp["A_log"].double())
    rep.add("y", bufs["yc"].out.view(2, B, Lc, d), y, S.TOL_Y, 2)
    _report(name, rep)


def fold_bound(inp, ref, bf16):
    """Elementwise bound of dxc + dxc2 against ``total`` = du + dx_dbl @ Wx, (2, B * Lc, d_in): fp32 storage the du bound
    per (direction, element); bf16 storage adds, per element, the bf16 matrix-core product of every chunk's partial rows
    (each term off by at most 2**-8 relative: bounded on the partials' magnitudes) and the bf16 storage of dxc2."""
    B, Lc, d = inp["B"], inp["Lc"], inp["d_in"]
    Wx = inp["Wx"].double()
    prod = torch.einsum("kmw,kwd->kmd", ref["dx_dbl"], Wx)
    total = ref["du"].reshape(2, B * Lc, d) + prod
    s = total.reshape(2, B, -1).abs().amax(-1).clamp_min(1.0)[:, :, None].expand(2, B, Lc * d).reshape(2, B * Lc, d)
    bound = S.TOL_DU * s
    if bf16:
        bound = bound + 2.0 ** -8 * torch.einsum("kmw,kwd->kmd", ref["slices"].abs().sum(0), Wx.abs()) + 2.0 ** -8 * prod.abs()
    return total, bound


@pytest.mark.parametrize("name", names("fold"))
def test_scan_bwd_xproj_fold_vs_fp64(lib, name):
    from fastvim_amd import _lib as L
    c, q = CASE_BY_NAME[name], Queries(lib)
    assert_keys(q, c)
    B, Lc, d, R = c["B"], c["Lc"], c["d"], c["R"]
    W, per_row = R + 2 * N, 2 * d * (N + R + 1)
    inp, ref = ref_of(name, 192)
    dev = Dev(c, inp)
    rows = B // c["nbb"]
    assert rows == B // q.nbb(B, Lc, R)

    def launch():
        bufs = dict(dxc=Buf(2 * B * Lc * d, d), dxc2=Buf(2 * B * Lc * d, d, TDT[c["dt"]]), dx_dbl=Buf(2 * 2 * B * Lc * W, 2 * B * Lc * W),
                    part=Buf(rows * per_row, per_row))
        rc = lib.fv_mixer_scan_bwd_xproj(L.ptr(dev.xc), L.ptr(dev.x_dbl), *[L.ptr(t) for t in dev.par], L.ptr(dev.dyc), L.ptr(dev.Wx[0]),
                                         L.ptr(dev.Wx[1]), L.ptr(dev.Wx2), L.ptr(bufs["dxc"].flat), L.ptr(bufs["dxc2"].flat),
                                         L.ptr(bufs["dx_dbl"].flat), L.ptr(bufs["part"].flat), *_shape_args(c), L.stream_of(dev.xc))
        return rc, bufs

    bufs = _twice(launch)
    for k in bufs:
        assert bufs[k].unwritten() == 0, f"{k} has unwritten elements"
    rep = S.Report()
    total, bound = fold_bound(inp, ref, c["dt"] == "bf16")
    got = (bufs["dxc"].out.double() + bufs["dxc2"].out.double()).view(2, B * Lc, d)
    rep.add_elementwise("dxc+dxc2", got, total, bound)
    rep.add("dx_dbl", bufs["dx_dbl"].out.view(2, 2, B * Lc, W), ref["slices"], S.TOL_DXDBL, 1)
    rep.add("rows", bufs["part"].out.view(rows, -1), S.group_rows(ref["rows"], c["nbb"]), S.TOL_PARAM, 1)
    _report(name, rep)


# ------------------------------------------------------------------------------------------------ refusals: an error code, no launch
def _refusal_case(B, Lc, d, R, dt):
    c = dict(name="refuse", kind="generic", B=B, Lc=Lc, d=d, R=R, dt=dt, dpd=False, seed=1, nbb=1, bwd=(("generic", dt, 24, "global"),))
    return c, Dev(c, S.make_inputs(B, Lc, d, R, dt == "bf16", 1, with_wx=True))


def test_generic_forward_refuses_rows_past_its_lds_stage(lib):
    """dt_rank > 48 stages Lc rows of 128 floats: 128 rows fill the 64 KiB (the generic case at Lc 128 runs it), 129 are an
    error -- no launch, the output stays as it was."""
    q = Queries(lib)
    c, dev = _refusal_case(1, 129, 64, 96, "f32")
    rc, bufs = launch_fwd(lib, q, c, dev, False, True)()
    torch.cuda.synchronize()
    assert rc != 0 and b"too long" in lib.fv_last_error()
    assert bufs["yc"].unwritten() == bufs["yc"].out.numel() and bufs["yc"].intact()


def test_backward_refuses_given_checkpoints_outside_the_chunked_kernel(lib):
    """Checkpoints of the forward launch are taken by the chunked kernel only: dt_rank > 48 (generic) and Lc <= 16 (short)
    answer with an error code and launch nothing."""
    q = Queries(lib)
    for B, Lc, d, R in ((2, 25, 64, 49), (2, 14, 64, 12)):
        c, dev = _refusal_case(B, Lc, d, R, "f32")
        c["nbb"] = q.nbb(B, Lc, R)
        c["bwd"] = (("generic", "f32", 24, "global"),) if R > 48 else (("short", "f32", 3, 14, True, c["nbb"]),)
        ck = torch.zeros(2 * B * cdiv(Lc, 4) * d * N, device="cuda")
        rc, bufs = launch_bwd(lib, q, c, dev, ck, False)[0]()
        torch.cuda.synchronize()
        assert rc != 0 and b"checkpoints" in lib.fv_last_error()
        assert all(bufs[k].unwritten() == bufs[k].out.numel() for k in ("dxc", "dx_dbl", "part"))


@pytest.mark.parametrize("B,Lc,d,R,dt", [(2, 17, 64, 12, "bf16"),       # Lc > 16
                                         (2, 14, 40, 12, "bf16"),       # d_inner no multiple of 32
                                         (2, 14, 800, 24, "bf16"),      # d_inner > 768
                                         (2, 14, 64, 49, "bf16"),       # dt_rank > 48
                                         (2, 14, 64, 12, "f32")])       # fp32 storage
def test_fused_forward_falls_back_where_it_is_not_built(lib, B, Lc, d, R, dt):
    """fv_mixer_xproj_scan_fwd_ok == 0: the C entry refuses without launching, and ``mixer_ops.xproj_scan_fwd`` hands the
    shape back to its caller (None), who runs x_proj and the scan separately."""
    from fastvim_amd import _lib as L
    from fastvim_amd import mixer_ops as M
    q = Queries(lib)
    assert not q.fused_ok(Lc, d, R, dt)
    c, dev = _refusal_case(B, Lc, d, R, dt)
    W = R + 2 * N
    x_dbl, yc = Buf(2 * B * Lc * W, W, TDT[dt]), Buf(2 * B * Lc * d, d)
    rc = lib.fv_mixer_xproj_scan_fwd(L.ptr(dev.xc), L.ptr(dev.Wx2), *[L.ptr(t) for t in dev.par], L.ptr(x_dbl.flat), L.ptr(yc.flat),
                                     *_shape_args(c), L.stream_of(dev.xc))
    torch.cuda.synchronize()
    assert rc != 0
    assert x_dbl.unwritten() == x_dbl.out.numel() and yc.unwritten() == yc.out.numel()
    p = dev.par
    assert M.xproj_scan_fwd(dev.xc, dev.Wx2.to(dev.xc.dtype), p[0], p[1], p[2], p[3], p[4], p[5]) is None
