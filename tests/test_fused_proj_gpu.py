"""The fused projection + norm launches, each on its own against the float64 stage references of ``fused_proj_ref.py``:
``fv_gemm_bf16_addnorm2``, ``fv_gemm_bf16_dgrad_addnorm_bwd2``, ``fv_mixer_combine_out_proj_addnorm`` (plain and ``_pk``),
``fv_mixer_conv_pool_bwd_dgrad`` (plain and ``_pk``) and ``fv_gemm_bf16_rowbias``, launched through the C ABI
(``fastvim_amd._lib.lib()``) into buffers of the test's own.

Stages (``fused_proj_ref.py`` derives every bound; nothing is measured from the kernels): the producer stage of the two
mixer launches against ``mixer_family_ref`` with the bounds of ``test_mixer_families_gpu.py`` (the conv partial rows per
workgroup); the product ``P64 = A @ W`` from the bf16 operands as stored -- in the producer launches A is the kernel's own
stored ``g`` or ``[x half of dxz written | z half given]``; the forward or backward epilogue; the second GEMM phase from the
kernel's own stored ``y`` / ``dx``.  Every stage's reference uses the launch's inputs and outputs of earlier stages only.

Every launch runs twice into freshly allocated buffers prefilled with -16384 (exact in bf16) and one 64-row tile longer than
needed: the two runs must be bit-identical, no sentinel may be left where the kernel must write, and the slack must still
hold it -- ``pw``, the conv partial rows and ``C2`` included.  The ``_pk`` forms must equal the plain ones bit for bit.

Shapes: M = 1 .. 1472 (row tiles with clamped dead rows; 1, 2, 4, 9 and 23 workgroups, i.e. remainder classes 1, 2, 4, 1, 7
of the XCD remap), K = 64 (one K tile, no prefetch) .. 768, A as a column half of a wider buffer, padded weight rows, the
DropPath scale per row / per 50 rows (straddling the 64-row tiles) / per launch with one sample at 0, N2 = 128 .. 768;
pooling-row tiles of 1 .. 4 rows in the producers.  Worst err / bound ratios seen on an MI355X are recorded in DESIGN.md
section 4; they are records, not thresholds.
"""
import ctypes

import pytest
import torch

import fused_proj_ref as R
import mixer_family_ref as MR
import norm_checks as N

pytestmark = pytest.mark.gpu

F64 = torch.float64
BF16, F32 = torch.bfloat16, torch.float32
SENT = -16384.0
NCOL, D_IN = 192, 384
EPS = 1e-5
PAD = 1000.0            # what the padding of a padded weight row holds: finite, and far off if it is ever multiplied
WORST = {}              # worst err / bound ratio per output over the module (printed by every test)


@pytest.fixture(scope="module")
def lib():
    import fastvim_amd.build as fb
    fb.build()
    from fastvim_amd import _lib
    return _lib.lib()


def _L():
    from fastvim_amd import _lib
    return _lib


class Out:
    """Output buffers of one launch: each (rows, width), prefilled with the sentinel, one 64-row tile of slack behind."""

    def __init__(self):
        self.bufs = {}

    def new(self, name, rows, width, dtype):
        n = rows * width
        flat = torch.full((n + R.TILE * width,), SENT, device="cuda", dtype=dtype)
        self.bufs[name] = (flat[:n].view(rows, width), flat[n:])
        return self.bufs[name][0]


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def twice(launch):
    """Run ``launch() -> Out`` twice; bit-identical runs, no sentinel left in an output, slack intact.  Returns the first
    run's outputs on the CPU (stats as 1-D)."""
    a, b = launch(), launch()
    torch.cuda.synchronize()
    res = {}
    for name, (va, sa) in a.bufs.items():
        vb, sb = b.bufs[name]
        assert torch.equal(_bits(va), _bits(vb)), f"{name}: two launches differ"
        assert bool((sa == SENT).all()) and bool((sb == SENT).all()), f"{name}: written past its end"
        assert not bool((va == SENT).any()), f"{name}: an element was left unwritten"
        res[name] = va.cpu().reshape(-1) if va.shape[1] == 1 else va.cpu()
    return res


def finish(rep, what):
    for k, v in rep.ratio.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print(what, {k: round(v, 3) for k, v in rep.ratio.items()})
    print("worst so far", {k: round(v, 3) for k, v in sorted(WORST.items())})
    assert rep, rep.msgs


def make_scale(B):
    """B distinct DropPath scales 1 / keep; one sample dropped (scale 0) when there are at least two."""
    s = 1.0 / (1.0 - 0.05 * (1 + torch.arange(B, dtype=F32) % 9))
    if B >= 2:
        s[B // 2] = 0.0
    return s


def padded_weight(W, pad):
    """(rows, cols) bf16 -> the same values as a view of a (rows, cols + pad) buffer whose padding holds PAD."""
    if not pad:
        return W.contiguous()
    buf = torch.full((W.shape[0], W.shape[1] + pad), PAD, dtype=W.dtype)
    buf[:, :W.shape[1]] = W
    return buf


def c_long(v):
    return ctypes.c_long(int(v))


# ------------------------------------------------------------------------------------------------ GEMM-fused forms
def _g(name, M, K, lda2=False, wpad=0, rps=None, dres=True, N2=0, fam="plain"):
    return dict(name=name, M=M, K=K, lda2=lda2, wpad=wpad, rps=rps, dres=dres, N2=N2, fam=fam)


# rps: None = no row_scale, "M" = one scale for the launch, else rows per scale
FWD_CASES = [
    _g("m1_k64", 1, 64),
    _g("m1_k384_half_pad_sM", 1, 384, True, 8, "M"),
    _g("m63_k128_pad_s1", 63, 128, False, 8, 1),
    _g("m64_k64_half_n2_128", 64, 64, True, 0, None, N2=128),
    _g("m65_k384_sM_offset", 65, 384, False, 0, "M", fam="offset"),
    _g("m100_k768_half_pad_s50", 100, 768, True, 8, 50),
    _g("m200_k384_pad_s50_n2_384", 200, 384, False, 8, 50, N2=384),
    _g("m200_k64_s50_zero_rows", 200, 64, False, 0, 50, fam="zero_rows"),
    _g("m513_k128_half_s1_zero_rows", 513, 128, True, 0, 1, fam="zero_rows"),
    _g("m513_k768_pad_sM_offset", 513, 768, False, 8, "M", fam="offset"),
    _g("m1472_k384_s50", 1472, 384, False, 0, 50),
    _g("m1472_k768_half_pad", 1472, 768, True, 8),
]
BWD_CASES = [
    _g("m1_k64_nodres", 1, 64, dres=False),
    _g("m1_k768_half_pad_sM_n2_128", 1, 768, True, 8, "M", N2=128),
    _g("m63_k128_half_s1", 63, 128, True, 0, 1),
    _g("m64_k384_pad_nodres_n2_384", 64, 384, False, 8, None, dres=False, N2=384),
    _g("m65_k64_s50_n2_128", 65, 64, False, 0, 50, N2=128),
    _g("m100_k768_half_pad_s50_n2_384", 100, 768, True, 8, 50, N2=384),
    _g("m200_k384_sM_nodres_n2_768", 200, 384, False, 0, "M", dres=False, N2=768),
    _g("m200_k128_half_pad_s1_zero_rows", 200, 128, True, 8, 1, fam="zero_rows"),
    _g("m513_k384_pad_s50_n2_128_offset", 513, 384, False, 8, 50, N2=128, fam="offset"),
    _g("m513_k64_half_n2_768", 513, 64, True, 0, None, N2=768),
    _g("m1472_k768_half_pad_s50_n2_384", 1472, 768, True, 8, 50, N2=384),
    _g("m1472_k128_sM_nodres", 1472, 128, False, 0, "M", dres=False),
]


def gemm_inputs(c, backward):
    """CPU inputs of a case.  residual / w / dres come from norm_checks.make_inputs ("plain", "zero_rows"); "offset" puts
    every residual row 30 of its standard deviations off zero, alternating in sign."""
    M, K = c["M"], c["K"]
    inp = N.make_inputs("zero_rows" if c["fam"] == "zero_rows" else "plain", 1, M, NCOL, True, seed=K)
    g = torch.Generator().manual_seed(100 * M + K + int(backward))
    rn = lambda *s: torch.randn(*s, generator=g)
    wide = rn(M, 2 * K if c["lda2"] else K).to(BF16)
    if c["fam"] == "zero_rows":
        wide[::7] = 0
    A = wide[:, K:] if c["lda2"] else wide          # the second column half of the wider buffer
    res = inp["residual"].clone()
    if c["fam"] == "offset":
        res += 30.0 * torch.where(torch.arange(M) % 2 == 0, 1.0, -1.0)[:, None]
    rps = M if c["rps"] == "M" else c["rps"]
    scale = None if rps is None else make_scale(-(-M // rps))
    t = dict(M=M, K=K, wide=wide, A=A, lda=wide.shape[1], res=res, w=inp["w"], scale=scale, rps=rps or 1,
             srow=R.row_scales(scale, rps, M), N2=c["N2"])
    if backward:
        Wkn = (rn(K, NCOL) * NCOL ** -0.5).to(BF16)                 # in_proj.weight as stored: (K, N)
        t["Wbuf"] = padded_weight(Wkn, c["wpad"])
        t["rstd"] = torch.rsqrt(res.double().square().mean(1) + EPS).float()
        t["dres"] = inp["dres"] if c["dres"] else None
        if c["N2"]:
            W2kn = (rn(NCOL, c["N2"]) * NCOL ** -0.5).to(BF16)      # out_proj.weight as stored: (192, N2)
            t["W2buf"], t["W2kn"] = padded_weight(W2kn, 8), W2kn
    else:
        Wnk = (rn(NCOL, K) * K ** -0.5).to(BF16)                    # out_proj.weight as stored: (N, K)
        Wkn = Wnk.t()
        t["Wbuf"] = padded_weight(Wnk, c["wpad"])
        if c["N2"]:
            W2nk = (rn(c["N2"], NCOL) * NCOL ** -0.5).to(BF16)      # in_proj.weight as stored: (N2, 192)
            t["W2buf"], t["W2kn"] = padded_weight(W2nk, 8), W2nk.t()
    t["Wkn"] = Wkn
    return t


def _dev(t, *keys):
    return {k: (t[k].cuda() if torch.is_tensor(t.get(k)) else None) for k in keys}


def launch_fwd(lib, t):
    L = _L()
    v = _dev(t, "wide", "Wbuf", "res", "w", "scale", "W2buf")
    M, K, N2 = t["M"], t["K"], t["N2"]
    A = v["wide"][:, t["lda"] - K:]

    def go():
        o = Out()
        y, ro, rs = o.new("y", M, NCOL, BF16), o.new("res_out", M, NCOL, F32), o.new("rstd", M, 1, F32)
        C2 = o.new("C2", M, N2, BF16) if N2 else None
        rc = lib.fv_gemm_bf16_addnorm2(
            L.ptr(A), L.ptr(v["Wbuf"]), L.ptr(v["res"]), L.ptr(v["w"]), L.ptr(v["scale"]), L.i32(t["rps"]), L.ptr(y), L.ptr(ro),
            L.ptr(rs), L.i32(M), L.i32(NCOL), L.i32(K), c_long(t["lda"]), c_long(v["Wbuf"].stride(0)), ctypes.c_float(EPS),
            L.ptr(v["W2buf"]), L.ptr(C2), L.i32(N2), c_long(v["W2buf"].stride(0) if N2 else 0), L.stream_of(A))
        L.check(rc, "gemm_bf16_addnorm2")
        return o
    return twice(go)


def launch_bwd(lib, t):
    L = _L()
    v = _dev(t, "wide", "Wbuf", "res", "rstd", "w", "scale", "dres", "W2buf")
    M, K, N2 = t["M"], t["K"], t["N2"]
    A = v["wide"][:, t["lda"] - K:]
    nb = lib.fv_gemm_bf16_dgrad_addnorm_blocks(L.i32(M))
    assert nb == -(-M // R.TILE)

    def go():
        o = Out()
        dx, dri, pw = o.new("dx", M, NCOL, BF16), o.new("dres_in", M, NCOL, F32), o.new("pw", nb, NCOL, F32)
        C2 = o.new("C2", M, N2, BF16) if N2 else None
        rc = lib.fv_gemm_bf16_dgrad_addnorm_bwd2(
            L.ptr(A), L.ptr(v["Wbuf"]), L.ptr(v["dres"]), L.ptr(v["res"]), L.ptr(v["rstd"]), L.ptr(v["w"]), L.ptr(v["scale"]),
            L.i32(t["rps"]), L.ptr(dx), L.ptr(dri), L.ptr(pw), L.i32(M), L.i32(NCOL), L.i32(K), c_long(t["lda"]),
            c_long(v["Wbuf"].stride(0)), L.ptr(v["W2buf"]), L.ptr(C2), L.i32(N2), c_long(v["W2buf"].stride(0) if N2 else 0),
            L.stream_of(A))
        L.check(rc, "gemm_bf16_dgrad_addnorm_bwd2")
        return o
    return twice(go), nb


def check_fwd_stages(t, out, A=None, res_out=None, C2=None):
    """The stages of a forward launch (``A`` / ``res_out`` / ``C2``: a replacement, for the defect tests)."""
    rep = R.Report()
    P, eps_x = R.product(t["A"] if A is None else A, t["Wkn"])
    R.check_forward(rep, P, eps_x, t["res"], t["srow"], t["w"], EPS, out["res_out"] if res_out is None else res_out,
                    out["rstd"], out["y"])
    if t["N2"]:
        R.check_second(rep, out["y"], t["W2kn"], out["C2"] if C2 is None else C2)
    return rep


def check_bwd_stages(t, out, nb, A=None, pw=None, C2=None):
    rep = R.Report()
    P, eps_x = R.product(t["A"] if A is None else A, t["Wkn"])
    R.check_backward(rep, P, eps_x, t["res"], t["rstd"], t["w"], t["dres"], t["srow"], out["dres_in"], out["dx"],
                     out["pw"] if pw is None else pw, R.gemm_pw_rows(t["M"], nb))
    if t["N2"]:
        R.check_second(rep, out["dx"], t["W2kn"], out["C2"] if C2 is None else C2)
    return rep


@pytest.mark.parametrize("c", FWD_CASES, ids=lambda c: c["name"])
def test_gemm_addnorm2_vs_fp64(lib, c):
    t = gemm_inputs(c, backward=False)
    out = launch_fwd(lib, t)
    finish(check_fwd_stages(t, out), "addnorm2 " + c["name"])


@pytest.mark.parametrize("c", BWD_CASES, ids=lambda c: c["name"])
def test_gemm_dgrad_addnorm_bwd2_vs_fp64(lib, c):
    t = gemm_inputs(c, backward=True)
    out, nb = launch_bwd(lib, t)
    finish(check_bwd_stages(t, out, nb), "dgrad_addnorm_bwd2 " + c["name"])


def test_gemm_forms_refuse_what_they_are_not_built_for(lib):
    """N != 192 or K no multiple of 64: FV_ERR_UNSUPPORTED (the caller runs the unfused launches), nothing written."""
    L = _L()
    for K, Nn in ((96, NCOL), (128, 128)):
        o = Out()
        A = torch.zeros(8, K, device="cuda", dtype=BF16)
        W = torch.zeros(Nn, K, device="cuda", dtype=BF16)
        res, w = torch.zeros(8, Nn, device="cuda"), torch.ones(Nn, device="cuda")
        y, ro, rs = o.new("y", 8, Nn, BF16), o.new("res_out", 8, Nn, F32), o.new("rstd", 8, 1, F32)
        rc = lib.fv_gemm_bf16_addnorm2(L.ptr(A), L.ptr(W), L.ptr(res), L.ptr(w), L.ptr(None), L.i32(1), L.ptr(y), L.ptr(ro), L.ptr(rs),
                                       L.i32(8), L.i32(Nn), L.i32(K), c_long(K), c_long(K), ctypes.c_float(EPS), L.ptr(None),
                                       L.ptr(None), L.i32(0), c_long(0), L.stream_of(A))
        assert rc != 0
        pw = o.new("pw", 1, Nn, F32)
        Wk = torch.zeros(K, Nn, device="cuda", dtype=BF16)
        rc = lib.fv_gemm_bf16_dgrad_addnorm_bwd2(L.ptr(A), L.ptr(Wk), L.ptr(None), L.ptr(res), L.ptr(torch.ones(8, device="cuda")),
                                                 L.ptr(w), L.ptr(None), L.i32(1), L.ptr(y), L.ptr(ro), L.ptr(pw), L.i32(8), L.i32(Nn),
                                                 L.i32(K), c_long(K), c_long(Nn), L.ptr(None), L.ptr(None), L.i32(0), c_long(0),
                                                 L.stream_of(A))
        assert rc != 0
        torch.cuda.synchronize()
        for name, (va, sa) in o.bufs.items():
            assert bool((va == SENT).all()) and bool((sa == SENT).all()), name


def test_stages_catch_defects_in_real_outputs(lib):
    """Applied in-process to real kernel outputs or inputs, each defect fails the stage meant to catch it -- and only after
    the unmodified outputs have passed."""
    t = gemm_inputs(_g("defects_fwd", 200, 384, False, 8, 50, N2=128), backward=False)
    out = launch_fwd(lib, t)
    assert check_fwd_stages(t, out)
    A0 = t["A"].clone()
    A0[:, -64:] = 0                                                   # the reference is fed an A without its last K tile
    rep = check_fwd_stages(t, out, A=A0)
    assert any(m.startswith("res_out") for m in rep.msgs) and rep.ratio["res_out"] > 100, rep.msgs
    rep = check_fwd_stages(t, out, res_out=out["res_out"].roll(1, 0))  # res_out shifted by one row
    assert any(m.startswith("res_out") for m in rep.msgs), rep.msgs
    bad = out["C2"].clone()
    bad[:, -8:] = 0                                                   # the last 8 columns of C2 zeroed
    rep = check_fwd_stages(t, out, C2=bad)
    assert [m[:2] for m in rep.msgs] == ["C2"], rep.msgs

    t = gemm_inputs(_g("defects_bwd", 200, 768, True, 8, 50, N2=384), backward=True)
    out, nb = launch_bwd(lib, t)
    assert check_bwd_stages(t, out, nb)
    A0 = t["A"].clone()
    A0[:, -64:] = 0
    rep = check_bwd_stages(t, out, nb, A=A0)
    assert any(m.startswith("dres_in") for m in rep.msgs) and any(m.startswith("pw") for m in rep.msgs), rep.msgs
    rep = check_bwd_stages(t, out, nb, pw=out["pw"][:-1])             # one workgroup's pw row dropped
    assert any("rows for" in m for m in rep.msgs), rep.msgs
    shifted = torch.cat([out["pw"][:1], out["pw"][2:], out["pw"][1:2]])   # ... or handed to the wrong workgroup
    rep = check_bwd_stages(t, out, nb, pw=shifted)
    assert [m[:2] for m in rep.msgs] == ["pw"], rep.msgs
    bad = out["C2"].clone()
    bad[:, -8:] = 0
    rep = check_bwd_stages(t, out, nb, C2=bad)
    assert [m[:2] for m in rep.msgs] == ["C2"], rep.msgs


# ------------------------------------------------------------------------------------------------ patch-embed epilogue
@pytest.mark.parametrize("M,Nn,K,period", [(21, 192, 768, 7), (392, 384, 768, 196), (130, 72, 40, 13)])
def test_gemm_rowbias_vs_fp64(lib, M, Nn, K, period):
    L = _L()
    g = torch.Generator().manual_seed(M + K)
    A = torch.randn(M, K, generator=g).to(BF16)
    W = (torch.randn(Nn, K, generator=g) * K ** -0.5).to(BF16)
    table = torch.randn(period, Nn, generator=g)
    v = dict(A=A.cuda(), W=W.cuda(), table=table.cuda())

    def go():
        o = Out()
        C = o.new("C", M, Nn, F32)
        rc = lib.fv_gemm_bf16_rowbias(L.ptr(v["A"]), L.ptr(v["W"]), L.ptr(C), L.ptr(v["table"]), L.i32(period), L.i32(M), L.i32(Nn),
                                      L.i32(K), c_long(K), c_long(K), c_long(Nn), L.stream_of(v["A"]))
        L.check(rc, "gemm_bf16_rowbias")
        return o
    out = twice(go)
    rep = R.Report()
    P, eps_x = R.product(A, W.t())
    R.check_rowbias(rep, P, eps_x, table, out["C"], tag="rowbias ")
    finish(rep, f"rowbias {M}x{Nn}x{K}")


# ------------------------------------------------------------------------------------------------ combine + out_proj + norm
def _m(B, rows, cols, tr, **kw):
    return dict(B=B, rows=rows, cols=cols, tr=tr, **kw)


COMBINE_CASES = [
    _m(1, 1, 1, False, ln=True, scale=False, wpad=0),
    _m(2, 1, 16, False, ln=True, scale=True, wpad=8),
    _m(1, 4, 16, False, ln=False, scale=False, wpad=0),
    _m(3, 5, 9, False, ln=True, scale=True, wpad=0),
    _m(2, 7, 9, True, ln=False, scale=True, wpad=8),
    _m(5, 2, 3, True, ln=True, scale=True, wpad=0),
    _m(2, 14, 14, False, ln=True, scale=True, wpad=8),
    _m(2, 14, 14, True, ln=True, scale=False, wpad=0, offset=True),       # pre-norm rows 30 sigma off zero
    _m(1, 16, 16, True, ln=False, scale=False, wpad=8),
]


def _mid(c):
    return "b{B}_{rows}x{cols}".format(**c) + ("_t" if c["tr"] else "") + "".join(
        "_" + k for k in ("ln", "scale", "offset", "dxc2", "nobias", "noD", "dres") if c.get(k)) + (
        f"_pad{c['wpad']}" if c.get("wpad") else "") + (f"_n2_{c['N2']}" if c.get("N2") else "")


def combine_inputs(c):
    B, rows, cols = c["B"], c["rows"], c["cols"]
    L_, M = rows * cols, B * rows * cols
    g = torch.Generator().manual_seed(17 * B + 5 * rows + cols + int(c["tr"]))
    rn = lambda *s: torch.randn(*s, generator=g)
    t = dict(xz=rn(B, L_, 2 * D_IN).to(BF16), skip=rn(B, L_, D_IN).to(BF16), yc=rn(2, B, rows, D_IN),
             ln_w=(1 + 0.1 * rn(D_IN)) if c["ln"] else None, ln_b=0.1 * rn(D_IN) if c["ln"] else None,
             res=rn(M, NCOL), w=1 + 0.1 * rn(NCOL), scale=make_scale(B) if c["scale"] else None, rps=L_, M=M)
    Wnk = (rn(NCOL, D_IN) * D_IN ** -0.5).to(BF16)
    t["Wnk"], t["Wbuf"], t["Wkn"] = Wnk, padded_weight(Wnk, c["wpad"]), Wnk.t()
    if c.get("offset"):
        # every pre-norm row o = 0.5 * (yc_f + yc_b + skip) gets a common offset of 30 of the largest row deviation (2 % on top)
        o = MR.combine_ref(t["xz"][..., D_IN:], t["skip"], t["yc"], t["ln_w"], t["ln_b"], EPS, rows, cols, 1, c["tr"])[0]
        t["yc"][0] += float(2 * 30 * 1.02 * o.std(-1).max())
    t["srow"] = R.row_scales(t["scale"], L_, M)
    return t


def launch_combine(lib, c, t, packed, check_ok=True):
    from fastvim_amd import mixer_ops as MO
    L = _L()
    v = _dev(t, "xz", "skip", "yc", "ln_w", "ln_b", "res", "w", "scale", "Wbuf")
    B, rows, cols, M = c["B"], c["rows"], c["cols"], t["M"]
    s_i, s_j = (1, rows) if c["tr"] else (cols, 1)
    if packed:
        Warg, ldw, fn = MO.pack_weight_frags_ref(t["Wnk"].contiguous()).contiguous().cuda(), D_IN, lib.fv_mixer_combine_out_proj_addnorm_pk
    else:
        Warg, ldw, fn = v["Wbuf"], v["Wbuf"].stride(0), lib.fv_mixer_combine_out_proj_addnorm
    assert not check_ok or lib.fv_mixer_combine_out_proj_addnorm_ok(L.i32(B), L.i32(rows), L.i32(cols), L.i32(1), L.i32(D_IN), L.i32(NCOL),
                                                                    L.i32(L.FV_BF16))

    def go():
        o = Out()
        gbuf = o.new("g", M, D_IN, BF16)
        mean = o.new("mean", M, 1, F32) if c["ln"] else None
        rln = o.new("rstd_ln", M, 1, F32) if c["ln"] else None
        y, ro, rs = o.new("y", M, NCOL, BF16), o.new("res_out", M, NCOL, F32), o.new("rstd", M, 1, F32)
        rc = fn(L.ptr(v["xz"]), L.ptr(v["skip"]), L.ptr(v["yc"]), L.ptr(v["ln_w"]), L.ptr(v["ln_b"]), ctypes.c_float(EPS), L.ptr(gbuf),
                L.ptr(mean), L.ptr(rln), L.i32(B), L.i32(rows), L.i32(cols), L.i32(s_i), L.i32(s_j), L.ptr(Warg), c_long(ldw),
                L.ptr(v["res"]), L.ptr(v["w"]), L.ptr(v["scale"]), L.i32(t["rps"]), L.ptr(y), L.ptr(ro), L.ptr(rs), ctypes.c_float(EPS),
                L.stream_of(v["xz"]))
        L.check(rc, "mixer_combine_out_proj_addnorm")
        return o
    return twice(go)


@pytest.mark.parametrize("c", COMBINE_CASES, ids=_mid)
def test_combine_out_proj_addnorm_vs_fp64(lib, c):
    t = combine_inputs(c)
    out = launch_combine(lib, c, t, packed=False)
    pk = launch_combine(lib, c, t, packed=True)
    for k in out:
        assert torch.equal(_bits(out[k]), _bits(pk[k])), f"{k}: the packed-weight form differs"
    B, rows, cols = c["B"], c["rows"], c["cols"]
    # ---- producer stage: g, mean, rstd_ln against combine_ref with the bounds of test_mixer_families_gpu.py (bf16 storage)
    o, g64, mean, rstd = MR.combine_ref(t["xz"][..., D_IN:], t["skip"], t["yc"], t["ln_w"], t["ln_b"], EPS, rows, cols, 1, c["tr"])
    if c.get("offset"):
        assert (o.mean(-1).abs() / o.std(-1)).min().item() >= 30.0
    errs = []
    MR.close(errs, "g", out["g"].view(B, rows * cols, D_IN), g64, 1e-5, True)
    if c["ln"]:
        MR.close(errs, "mean", out["mean"], mean, 1e-5, elementwise_scale=True)
        MR.close(errs, "rstd_ln", out["rstd_ln"], rstd, 1e-5, elementwise_scale=True)
    assert not errs, errs
    # ---- product of the stored g, then the forward epilogue
    rep = R.Report()
    P, eps_x = R.product(out["g"], t["Wkn"])
    R.check_forward(rep, P, eps_x, t["res"], t["srow"], t["w"], EPS, out["res_out"], out["rstd"], out["y"], tag="combine ")
    finish(rep, "combine " + _mid(c))


# ------------------------------------------------------------------------------------------------ conv + pool adjoint + dgrad
CONVPOOL_CASES = [
    _m(1, 1, 14, False, scaling=1.0),
    _m(2, 2, 16, True, dxc2=True, scaling=0.25, dres=True, scale=True, N2=128),
    _m(3, 3, 14, False, dxc2=True, nobias=True, scaling=1.0, dres=True, N2=384),
    _m(1, 4, 16, False, noD=True, scaling=0.5, scale=True),
    _m(2, 5, 14, True, dxc2=True, scaling=1.0, dres=True, scale=True, N2=384, wpad=8),
    _m(3, 5, 16, False, scaling=0.25, dres=True, N2=128, wpad=8),
    _m(2, 14, 14, False, dxc2=True, scaling=1.0, dres=True, scale=True, N2=384),
    _m(1, 14, 16, True, dxc2=True, scaling=1.0, scale=True, wpad=8),
    _m(2, 16, 14, False, nobias=True, scaling=1.0, dres=True, N2=128),
    _m(1, 16, 16, True, nobias=True, noD=True, scaling=0.25, dres=True, N2=128),
]


def convpool_inputs(c):
    B, rows, cols = c["B"], c["rows"], c["cols"]
    L_, M = rows * cols, B * rows * cols
    g = torch.Generator().manual_seed(29 * B + 7 * rows + cols + int(c["tr"]))
    rn = lambda *s: torch.randn(*s, generator=g)
    nob, noD = c.get("nobias"), c.get("noD")
    t = dict(xz=rn(B, L_, 2 * D_IN).to(BF16), d_o=rn(B, L_, D_IN).to(BF16), dxc=rn(2, B, rows, D_IN),
             dxc2=rn(2, B, rows, D_IN).to(BF16) if c.get("dxc2") else None, dz=rn(B, L_, D_IN).to(BF16),
             cw=0.5 * rn(D_IN, 4), cwb=0.5 * rn(D_IN, 4), cb=None if nob else 0.2 * rn(D_IN), cbb=None if nob else 0.2 * rn(D_IN),
             D=None if noD else 1 + 0.1 * rn(D_IN), Db=None if noD else 1 + 0.1 * rn(D_IN),
             res=rn(M, NCOL), w=1 + 0.1 * rn(NCOL), dres=rn(M, NCOL) if c.get("dres") else None,
             scale=make_scale(B) if c.get("scale") else None, rps=L_, M=M, N2=c.get("N2", 0))
    t["rstd"] = torch.rsqrt(t["res"].double().square().mean(1) + EPS).float()
    W_in = (rn(2 * D_IN, NCOL) * NCOL ** -0.5).to(BF16)               # in_proj.weight as stored: (768, 192)
    t["Wkn"], t["Wt"] = W_in, W_in.t().contiguous()
    t["Wtbuf"] = padded_weight(t["Wt"], c.get("wpad", 0))
    if t["N2"]:
        t["W2kn"] = (rn(NCOL, t["N2"]) * NCOL ** -0.5).to(BF16)
        t["W2buf"] = padded_weight(t["W2kn"], c.get("wpad", 0))
    t["srow"] = R.row_scales(t["scale"], L_, M)
    return t


def launch_convpool(lib, c, t, packed, check_ok=True):
    from fastvim_amd import mixer_ops as MO
    L = _L()
    v = _dev(t, "xz", "d_o", "dxc", "dxc2", "dz", "cw", "cwb", "cb", "cbb", "D", "Db", "res", "rstd", "w", "dres", "scale", "Wtbuf", "W2buf")
    B, rows, cols, M, N2 = c["B"], c["rows"], c["cols"], t["M"], t["N2"]
    s_i, s_j = (1, rows) if c["tr"] else (cols, 1)
    if packed:
        Warg, ldwt, fn = MO.pack_weight_frags_ref(t["Wt"]).contiguous().cuda(), 2 * D_IN, lib.fv_mixer_conv_pool_bwd_dgrad_pk
    else:
        Warg, ldwt, fn = v["Wtbuf"], v["Wtbuf"].stride(0), lib.fv_mixer_conv_pool_bwd_dgrad
    assert not check_ok or lib.fv_mixer_conv_pool_bwd_dgrad_ok(L.i32(B), L.i32(rows), L.i32(cols), L.i32(1), L.i32(D_IN), L.i32(NCOL),
                                                               L.i32(0), L.i32(L.FV_BF16))
    nb = lib.fv_mixer_conv_pool_bwd_dgrad_blocks(L.i32(B), L.i32(rows))
    assert nb == B * -(-rows // 4)

    def go():
        o = Out()
        dxz = o.new("dxz", M, 2 * D_IN, BF16)
        dxz[:, D_IN:] = v["dz"].view(M, D_IN)           # the z half is combine_bwd's output; the x half holds the sentinel
        part, pw = o.new("part", nb, 12 * D_IN, F32), o.new("pw", nb, NCOL, F32)
        dx, dri = o.new("dx", M, NCOL, BF16), o.new("dres_in", M, NCOL, F32)
        C2 = o.new("C2", M, N2, BF16) if N2 else None
        rc = fn(L.ptr(v["xz"]), L.ptr(v["d_o"]), L.ptr(v["dxc"]), L.ptr(v["dxc2"]), L.ptr(v["cw"]), L.ptr(v["cb"]), L.ptr(v["cwb"]),
                L.ptr(v["cbb"]), L.ptr(v["D"]), L.ptr(v["Db"]), L.ptr(dxz), L.ptr(part), L.i32(B), L.i32(rows), L.i32(cols), L.i32(s_i),
                L.i32(s_j), ctypes.c_float(c["scaling"]), L.ptr(Warg), c_long(ldwt), L.ptr(v["dres"]), L.ptr(v["res"]), L.ptr(v["rstd"]),
                L.ptr(v["w"]), L.ptr(v["scale"]), L.i32(t["rps"]), L.ptr(dx), L.ptr(dri), L.ptr(pw), L.ptr(v["W2buf"]), L.ptr(C2),
                L.i32(N2), c_long(v["W2buf"].stride(0) if N2 else 0), L.stream_of(v["xz"]))
        L.check(rc, "mixer_conv_pool_bwd_dgrad")
        return o
    return twice(go), nb


@pytest.mark.parametrize("c", CONVPOOL_CASES, ids=_mid)
def test_conv_pool_bwd_dgrad_vs_fp64(lib, c):
    t = convpool_inputs(c)
    out, nb = launch_convpool(lib, c, t, packed=False)
    pk, _ = launch_convpool(lib, c, t, packed=True)
    for k in out:
        assert torch.equal(_bits(out[k]), _bits(pk[k])), f"{k}: the packed-weight form differs"
    B, rows, cols, tr = c["B"], c["rows"], c["cols"], c["tr"]
    L_ = rows * cols
    dxz = out["dxz"].view(B, L_, 2 * D_IN)
    assert torch.equal(_bits(dxz[..., D_IN:]), _bits(t["dz"])), "the z half of dxz was touched"
    # ---- producer stage: the x half of dxz, and the conv partial row of every workgroup against the gradient of the terms
    #      of L = <d_o, 0.5 skip> + <dxc + dxc2, xc> that belong to ITS pooling rows (bounds of test_mixer_families_gpu.py)
    zD = torch.zeros(D_IN)
    D, Db = (zD, zD) if t["D"] is None else (t["D"], t["Db"])          # no D: no skip term (its gradient is not compared)
    x = t["xz"][..., :D_IN]
    ref = lambda b, d_o, dxc, dxc2: MR.conv_pool_adjoint_ref(x[b:b + 1], t["cw"], t["cb"], t["cwb"], t["cbb"], D, Db, d_o, dxc, rows, cols,
                                                             1, False, c["scaling"], tr, dxc2=dxc2)
    errs = []
    dx64 = torch.cat([ref(b, t["d_o"][b:b + 1], t["dxc"][:, b:b + 1], None if t["dxc2"] is None else t["dxc2"][:, b:b + 1])[0]
                      for b in range(B)])
    MR.close(errs, "dxz x half", dxz[..., :D_IN], dx64, 2e-5, True)
    grp = MR.pooled_index_of_mem(rows, cols, 1, tr)
    d = D_IN
    seg = dict(dw=(0, 4 * d), dw_b=(4 * d, 8 * d), db=(8 * d, 9 * d), db_b=(9 * d, 10 * d), dD=(10 * d, 11 * d), dD_b=(11 * d, 12 * d))
    for wg in range(nb):
        b, i0 = divmod(wg, -(-rows // 4))
        own = (torch.arange(rows) // 4 == i0)
        d_o = t["d_o"][b:b + 1].double() * own[grp][None, :, None]
        dxc = t["dxc"][:, b:b + 1].double() * own[None, None, :, None]
        dxc2 = None if t["dxc2"] is None else t["dxc2"][:, b:b + 1].double() * own[None, None, :, None]
        part = ref(b, d_o, dxc, dxc2)[1]
        for k, (lo, hi) in seg.items():
            if (k in ("db", "db_b") and t["cb"] is None) or (k in ("dD", "dD_b") and t["D"] is None):
                continue
            MR.close(errs, f"workgroup {wg} {k}", out["part"][wg, lo:hi], part[lo:hi], 1e-4)
    assert not errs, errs
    # ---- product of [x half written | z half given], the backward epilogue (pw per workgroup), the second phase
    rep = R.Report()
    P, eps_x = R.product(out["dxz"], t["Wkn"])
    R.check_backward(rep, P, eps_x, t["res"], t["rstd"], t["w"], t["dres"], t["srow"], out["dres_in"], out["dx"], out["pw"],
                     R.pooling_tile_rows(B, rows, cols, tr), tag="convpool ")
    if t["N2"]:
        R.check_second(rep, out["dx"], t["W2kn"], out["C2"], tag="convpool ")
    finish(rep, "convpool " + _mid(c))


def test_producer_launches_refuse_shapes_they_are_not_built_for(lib):
    L = _L()
    i = L.i32
    assert not lib.fv_mixer_combine_out_proj_addnorm_ok(i(1), i(2), i(17), i(1), i(D_IN), i(NCOL), i(L.FV_BF16))     # cols > 16
    assert not lib.fv_mixer_combine_out_proj_addnorm_ok(i(1), i(2), i(14), i(2), i(D_IN), i(NCOL), i(L.FV_BF16))     # tpp 2
    assert not lib.fv_mixer_conv_pool_bwd_dgrad_ok(i(1), i(2), i(15), i(1), i(D_IN), i(NCOL), i(0), i(L.FV_BF16))    # cols 15
    assert not lib.fv_mixer_conv_pool_bwd_dgrad_ok(i(1), i(2), i(14), i(1), i(D_IN), i(NCOL), i(1), i(L.FV_BF16))    # max pooling
    # the entry point itself: an error code and a message, nothing launched
    c = _m(1, 2, 15, False, scaling=1.0)
    with pytest.raises(RuntimeError, match="shape not built"):
        launch_convpool(lib, c, convpool_inputs(c), packed=False, check_ok=False)
    c = _m(1, 2, 17, False, ln=True, scale=False, wpad=0)
    with pytest.raises(RuntimeError, match="shape not built"):
        launch_combine(lib, c, combine_inputs(c), packed=False, check_ok=False)
