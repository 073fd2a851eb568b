"""The add + norm HIP kernels (``csrc/norm.hip``) against an unrounded fp64 reference, row by row: every width
branch of the dispatch, ragged row counts, the second pass of the persistent loop, the option forms the models
call, the saved statistics, and bitwise structure checks.  Bounds and their derivation: ``norm_checks.py``;
``test_norm_checks_cpu.py`` shows that each of them can fail.

Which kernel template a test reaches (dispatch of ``fv_add_norm_fwd`` / ``fv_add_norm_bwd``; extend this table and
``TEMPLATES`` / ``WIDTHS`` below when the dispatch changes).  "rows/step" is what one wave covers per trip of its
grid-stride loop; the grid is capped at ``4 * fv_add_norm_blocks(M)`` waves (8192), so the loop repeats only above
``8192 * rows/step`` rows.

    template              rows/step  widths here                  row counts here
    fwd3/bwd3<16>         8          192                          1..257, 131077 (3 trips)
    fwd3/bwd3<32>         4          384                          1..257, 65541
    fwd3/bwd3<64>         2          768                          1..257, 32773
    generic MAXK=1        4          4, 32, 252, 256              1..257, 65541 (at 252)
    generic MAXK=2        2          260, 512                     1..257, 32773 (at 260)
    generic MAXK=4        1          516, 1024                    1..257, 16389 (at 516)
    generic MAXK=8        1          1028, 1536, 2044, 2048       1..257, 16389 (at 1028)
    host-side refusal     -          30, 2052, row_scale length, LayerNorm without a mean buffer

The fwd3/bwd3 kernels load row ``M - 1`` again for the dead row slots of a wave's last step ("clamped" slots); every
row count that is not a multiple of rows/step has some.  The generic kernels mask columns ``c < N`` in their last
256-column step; every width that is not a multiple of 256 has a partly filled one.
"""
import ctypes

import pytest
import torch

import norm_checks as nc

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64

WIDTHS = (192, 384, 768, 4, 32, 252, 256, 260, 512, 516, 1024, 1028, 1536, 2044, 2048)
# template -> (width that reaches it, rows per wave step): norm.hip, RPW * RU = (64 / LPR) * 2 in add_norm_fwd3/bwd3_kernel<LPR>
# with LPR = N / 12, and RU = 4 / 2 / 1 / 1 at MAXK = 1 / 2 / 4 / 8 in add_norm_fwd/bwd_kernel<MAXK>
TEMPLATES = {"k3_16": (192, 8), "k3_32": (384, 4), "k3_64": (768, 2),
             "maxk1": (252, 4), "maxk2": (260, 2), "maxk4": (516, 1), "maxk8": (1028, 1)}
ROWS_PER_STEP = {N: rps for N, rps in TEMPLATES.values()}
# (B, L) with B >= 2 distinct samples wherever M allows
SMALL_ROWS = ((1, 1), (2, 1), (3, 1), (5, 1), (7, 1), (2, 4), (3, 3), (17, 1), (9, 7), (257, 1))
KINDS = ("rms", "ln")


def _lib():
    from fastvim_amd import _lib as L
    return L


def run_kernel(inp, rms, *, prenorm=True, residual_in_fp32=True, out_dtype=None, dy=True, dres=True, to="cpu"):
    """The op through ``rms_norm_fn`` (RMSNorm without bias) / ``layer_norm_fn`` on (B, L, N) tensors, forward and
    backward; returns the (M, N) / (N,) outputs on device ``to`` (None entries for absent ones)."""
    from fastvim_amd.layernorm import layer_norm_fn, rms_norm_fn
    M, N = inp["x"].shape
    B = inp["B"]
    g = lambda t, grad=False: None if t is None else t.detach().to(DEV, copy=True).requires_grad_(grad)
    sh = lambda t: None if t is None else t.detach().to(DEV, copy=True).reshape(B, M // B, N)
    x = sh(inp["x"]).requires_grad_()
    res = sh(inp["residual"])
    if res is not None:
        res.requires_grad_()
    w, b, rs = g(inp["w"], True), g(inp["b"], True), g(inp["row_scale"])
    if rms and b is None:
        out = rms_norm_fn(x, w, None, residual=res, prenorm=prenorm, residual_in_fp32=residual_in_fp32,
                          eps=inp["eps"], row_scale=rs, out_dtype=out_dtype)
    else:
        out = layer_norm_fn(x, w, b, residual=res, eps=inp["eps"], prenorm=prenorm,
                            residual_in_fp32=residual_in_fp32, is_rms_norm=rms, row_scale=rs, out_dtype=out_dtype)
    y, r = out if prenorm else (out, None)
    assert y.shape == x.shape and (r is None or r.shape == x.shape)
    tensors, grads = [], []
    if dy:
        tensors.append(y)
        grads.append(sh(inp["dy"]))
    if dres and prenorm:
        tensors.append(r)
        grads.append(sh(inp["dres"]))
    torch.autograd.backward(tensors, grads)
    o2 = lambda t: None if t is None else t.detach().reshape(-1, N).to(to)
    o1 = lambda t: None if t is None else t.detach().to(to)
    return {"y": o2(y), "r": o2(r), "dx": o2(x.grad), "dresidual": o2(res.grad) if res is not None else None,
            "dw": o1(w.grad), "db": o1(b.grad) if b is not None else None}


def _ctx(msgs, **kw):
    return " ".join(f"{k}={v}" for k, v in kw.items()) + ": " + "; ".join(msgs)


# ------------------------------------------------------------------------------------------- small and ragged rows
@pytest.mark.parametrize("xdt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", WIDTHS)
def test_small_ragged_rows(N, kind, xdt):
    """Every width branch x M in {1, 2, 3, 5, 7, 8, 9, 17, 63, 257}: fp32 residual, prenorm, per-sample row_scale,
    both upstream gradients; every output row-wise against fp64."""
    rms = kind == "rms"
    fails = []
    for B, Ltok in SMALL_ROWS:
        inp = nc.make_inputs("plain", B, Ltok, N, rms, xdt=xdt)
        ref = nc.reference_of(inp, rms)
        out = run_kernel(inp, rms)
        assert out["y"].dtype == xdt and out["r"].dtype == F32 and out["dx"].dtype == xdt
        assert out["dresidual"].dtype == F32
        msgs = nc.check_all(out, ref, inp["b"])
        if msgs:
            fails.append(_ctx(msgs, N=N, M=B * Ltok, kind=kind))
    assert not fails, "\n".join(fails)


# --------------------------------------------------------------------------- second pass of the persistent loop
def _two_pass_rows(N):
    """M = 2 * waves * rows_per_step + 5 with the wave cap read from the library; returns (M, rows of one pass)."""
    L = _lib()
    rps = ROWS_PER_STEP[N]
    waves_cap = 4 * L.lib().fv_add_norm_blocks(L.i32(1 << 30))
    M = 2 * waves_cap * rps + 5
    waves = 4 * L.lib().fv_add_norm_blocks(L.i32(M))
    # a change of the cap (or of rows per step) must not silently turn this back into a one-pass test
    assert M > waves * rps, (M, waves, rps)
    return M, waves * rps


def _samples(M):
    """Smallest divisor of M in 3..64 (B distinct row_scale values, one of them 0), else one sample per row."""
    for d in range(3, 65):
        if M % d == 0:
            return d
    return M


def _hot_rows(M, P):
    """First row, last row and its neighbour (the rows next to every clamped slot: the dead slots of a wave's last
    step all reload row M - 1), last row of the first pass, first rows of the second, and of the third pass."""
    return sorted({r for r in (0, 1, M - 2, M - 1, P - 1, P, P + 1, 2 * P - 1, 2 * P) if 0 <= r < M})


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tmpl", sorted(TEMPLATES))
def test_persistent_loop_second_pass(tmpl, kind):
    """Each kernel template at a row count where every wave walks its grid-stride loop at least twice
    (131077 x 192 is the largest); dense gradients, fp64 reference computed on the GPU with plain torch ops."""
    N = TEMPLATES[tmpl][0]
    rms = kind == "rms"
    M, P = _two_pass_rows(N)
    B = _samples(M)
    inp = nc.make_inputs("plain", B, M // B, N, rms)
    assert inp["row_scale"][0] == 0 and inp["row_scale"].unique().numel() >= min(B, 3)
    ref = nc.reference_of(inp, rms, device=DEV)
    out = run_kernel(inp, rms, to=DEV)
    msgs = nc.check_all(out, ref, inp["b"])
    assert not msgs, _ctx(msgs, template=tmpl, N=N, M=M, B=B, kind=kind, rows_per_pass=P)
    # fixed-order reductions: the same call again gives the same bits
    out2 = run_kernel(inp, rms, to=DEV)
    for k, v in out.items():
        assert v is None or torch.equal(v, out2[k]), f"{k} differs between two identical calls (N={N}, M={M})"


def _few_hot_case(N, rms, B, Ltok, P, where):
    M = B * Ltok
    hot = _hot_rows(M, P)
    mask = torch.zeros(M, 1)
    mask[hot] = 1
    cold = (mask[:, 0] == 0).to(where)
    fails = []
    for with_dres in (True, False):
        inp = nc.make_inputs("plain", B, Ltok, N, rms, seed=3)
        inp["dy"] = inp["dy"] * mask
        ref = nc.reference_of(inp, rms, dres=with_dres, device=None if where == "cpu" else where)
        out = run_kernel(inp, rms, dres=with_dres, to=where)
        # dw / db: the scale sum_rows |dy * xhat| has len(hot) addends, one missing or doubled row is an error of order 1
        msgs = nc.check_all(out, ref, inp["b"])
        sc = nc.rows_scale(inp["row_scale"], M).to(where)
        if with_dres:
            dres = inp["dres"].to(where)
            want_dres, want_dx = dres, dres * sc[:, None]          # one fp32 multiply = rounded once
        else:
            want_dres = want_dx = torch.zeros(M, N, device=where)
        if not torch.equal(out["dresidual"][cold], want_dres[cold]):
            bad = (out["dresidual"] != want_dres).any(1) & cold
            msgs.append(f"dresidual != dres exactly on rows without dy: rows {bad.nonzero().flatten()[:8].tolist()}")
        if not torch.equal(out["dx"][cold], want_dx[cold]):
            bad = (out["dx"] != want_dx).any(1) & cold
            msgs.append(f"dx != dres * row_scale exactly on rows without dy: rows {bad.nonzero().flatten()[:8].tolist()}")
        if msgs:
            fails.append(_ctx(msgs, N=N, M=M, hot=hot, dres=with_dres))
    return fails


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tmpl", sorted(TEMPLATES))
def test_few_hot_gradients_small(tmpl, kind):
    """dy zero except on a handful of rows, M in {7, 9, 257}: dw / db equal the fp64 sum over those few rows, every
    other row's dresidual is exactly dres and dx exactly dres * row_scale (0 without dres)."""
    N, rps = TEMPLATES[tmpl]
    fails = []
    for B, Ltok in ((7, 1), (3, 3), (257, 1)):
        fails += _few_hot_case(N, kind == "rms", B, Ltok, 4 * rps, "cpu")   # P: one block's rows, a wave boundary
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tmpl", sorted(TEMPLATES))
def test_few_hot_gradients_second_pass(tmpl, kind):
    """The same at the large shapes: hot rows at both ends, on both sides of every pass boundary and at the tail."""
    N = TEMPLATES[tmpl][0]
    M, P = _two_pass_rows(N)
    B = _samples(M)
    fails = _few_hot_case(N, kind == "rms", B, M // B, P, DEV)
    assert not fails, "\n".join(fails)


# --------------------------------------------------------------------------------------------------- input families
def _family_cases():
    for family in nc.FAMILIES:
        for kind in KINDS:
            if nc.family_applies(family, kind == "rms"):
                yield family, kind


@pytest.mark.parametrize("N", [192, 768, 260, 1028])
@pytest.mark.parametrize("family,kind", list(_family_cases()))
def test_input_families(family, kind, N):
    rms = kind == "rms"
    fails = []
    for B, Ltok in ((9, 7), (257, 1)):
        M = B * Ltok
        inp = nc.make_inputs(family, B, Ltok, N, rms)
        ref = nc.reference_of(inp, rms)
        out = run_kernel(inp, rms)
        msgs = nc.check_all(out, ref, inp["b"])
        for k, v in out.items():
            if v is not None and not torch.isfinite(v).all():
                msgs.append(f"{k} has non-finite values")
        if family == "zero_rows":
            want = torch.zeros(N) if inp["b"] is None else inp["b"]
            if not torch.equal(out["y"][::7], want.expand(len(out["y"][::7]), N)):
                msgs.append("y of an all-zero row is not exactly the bias (or 0)")
        if family == "scaled_eps0":
            # power-of-two scaling of a row commutes with every fp32 operation of the kernel while nothing under- or
            # overflows (squares reach 2^+-80), and the reciprocal square root sees the same mantissa and exponent
            # parity or one power of two less: y of a row and of the row * 2^k are the same bits
            base = dict(inp, x=inp["x"] / inp["pow2"], residual=inp["residual"] / inp["pow2"])
            y0 = run_kernel(base, rms)["y"]
            if not torch.equal(out["y"], y0):
                bad = (out["y"] != y0).any(1).nonzero().flatten()
                k = torch.log2(inp["pow2"][bad[:8], 0]).tolist()
                msgs.append(f"y(row * 2^k) != y(row) bitwise at eps = 0 on {len(bad)} rows, first {bad[:8].tolist()} with k = {k}")
        if msgs:
            fails.append(_ctx(msgs, family=family, N=N, M=M, kind=kind))
    assert not fails, "\n".join(fails)


# ----------------------------------------------------------------------------------------------------- option matrix
# the call forms of fastvim_amd/fastvim.py and mamba_simple*.py: x dtype, residual dtype (None = no residual), ...
FORMS = {
    "nores_res_fp32": dict(xdt=BF16, res=None, residual_in_fp32=True, scale=True),
    "nores_res_native": dict(xdt=BF16, res=None, residual_in_fp32=False, scale=False),
    "first_block": dict(xdt=F32, res=None, residual_in_fp32=True, prenorm=False, scale=False, out_dtype=BF16),
    "res_fp32": dict(xdt=F32, res=F32),
    "res_fp32_x_bf16_noscale": dict(xdt=BF16, res=F32, scale=False),
    "res_bf16_x_bf16": dict(xdt=BF16, res=BF16, residual_in_fp32=False),
    "norm_f": dict(xdt=F32, res=F32, prenorm=False),
    "out_bf16": dict(xdt=F32, res=F32, out_dtype=BF16),
    "grad_y_only": dict(xdt=F32, res=F32, dres=False),
    "grad_residual_only": dict(xdt=F32, res=F32, dy=False),
}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [192, 384, 260])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_option_matrix(form, N, kind):
    from oracle import fused_add_norm_oracle
    f = dict(dict(residual_in_fp32=True, prenorm=True, scale=True, out_dtype=None, dy=True, dres=True), **FORMS[form])
    rms = kind == "rms"
    B, Ltok = 9, 7
    res_out_dt = f["res"] if f["res"] is not None else (F32 if f["residual_in_fp32"] else f["xdt"])
    inp = nc.make_inputs("plain", B, Ltok, N, rms, xdt=f["xdt"], res_dt=res_out_dt, with_scale=f["scale"])
    if f["res"] is None:
        inp["residual"] = None
    y_dt = f["out_dtype"] or f["xdt"]
    inp["dy"] = inp["dy"].to(y_dt)
    dres = f["dres"] and f["prenorm"]
    ref = nc.reference_of(inp, rms, dy=f["dy"], dres=dres)
    out = run_kernel(inp, rms, prenorm=f["prenorm"], residual_in_fp32=f["residual_in_fp32"], out_dtype=f["out_dtype"],
                     dy=f["dy"], dres=dres)
    # dtypes and shapes by the oracle's rules
    sh = lambda t: None if t is None else t.reshape(B, Ltok, N)
    o = fused_add_norm_oracle(sh(inp["x"]), inp["w"], inp["b"], sh(inp["residual"]), inp["eps"], f["prenorm"],
                              f["residual_in_fp32"], rms, row_scale=inp["row_scale"], out_dtype=f["out_dtype"])
    oy, orr = o if f["prenorm"] else (o, None)
    assert out["y"].dtype == oy.dtype == y_dt and out["y"].numel() == oy.numel()
    if f["prenorm"]:
        assert out["r"].dtype == orr.dtype == res_out_dt
    else:
        assert out["r"] is None
    assert out["dx"].dtype == f["xdt"] and out["dw"].dtype == F32
    if f["res"] is not None:
        assert out["dresidual"].dtype == f["res"]
    # the one derived allowance: residual_out stored in bf16 AND rounded by the store (a sum or a scaled x)
    stored_r_bf16 = form == "res_bf16_x_bf16"
    msgs = nc.check_all(out, ref, inp["b"], stored_r_bf16=stored_r_bf16)
    assert not msgs, _ctx(msgs, form=form, N=N, M=B * Ltok, kind=kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [192, 384, 260])
def test_noncontiguous_x_and_expanded_dy(N, kind):
    """x is a column slice of a wider tensor, dy arrives as a stride-0 expansion (the gradient of a mean over tokens)."""
    from fastvim_amd.layernorm import layer_norm_fn
    rms = kind == "rms"
    B, Ltok = 9, 7
    inp = nc.make_inputs("plain", B, Ltok, N, rms)
    wide = torch.randn(B, Ltok, N + 24, generator=torch.Generator().manual_seed(N))
    wide[..., 8:8 + N] = inp["x"].reshape(B, Ltok, N)
    wide_g = wide.to(DEV).requires_grad_()
    x = wide_g[..., 8:8 + N]
    assert not x.is_contiguous()
    res = inp["residual"].to(DEV).reshape(B, Ltok, N).requires_grad_()
    w = inp["w"].to(DEV).requires_grad_()
    b = inp["b"].to(DEV).requires_grad_() if inp["b"] is not None else None
    y, r = layer_norm_fn(x, w, b, residual=res, eps=inp["eps"], prenorm=True, residual_in_fp32=True,
                         is_rms_norm=rms, row_scale=inp["row_scale"].to(DEV))
    seen = []
    y.register_hook(lambda g: seen.append(g))
    gy = inp["dy"].reshape(B, Ltok, N)[:, 0].to(DEV)
    # mean over tokens as sum / L: the sum's backward is an expand(), a stride-0 view, and nothing after it copies
    loss = (y.sum(1) * (1.0 / Ltok) * gy).sum() + (r * inp["dres"].to(DEV).reshape(B, Ltok, N)).sum()
    loss.backward()
    assert len(seen) == 1 and seen[0].stride(1) == 0, "premise: dy reaches the op as an expanded tensor"
    inp["dy"] = seen[0].detach().cpu().reshape(-1, N).clone()
    ref = nc.reference_of(inp, rms)
    c = lambda t: t.detach().cpu()
    out = {"y": c(y).reshape(-1, N), "r": c(r).reshape(-1, N), "dx": c(wide_g.grad[..., 8:8 + N]).reshape(-1, N),
           "dresidual": c(res.grad).reshape(-1, N), "dw": c(w.grad), "db": c(b.grad) if b is not None else None}
    msgs = nc.check_all(out, ref, inp["b"])
    assert not msgs, _ctx(msgs, N=N, kind=kind)
    outside = c(wide_g.grad).clone()
    outside[..., 8:8 + N] = 0
    assert outside.abs().max().item() == 0.0, "gradient written outside the slice"


# -------------------------------------------------------------------------------------------------- saved statistics
def _c_fwd(x, res, w, b, rs, rows_per_scale, eps, rms, with_mean=True):
    """fv_add_norm_fwd through ctypes; returns (rc, y, residual_out, mean, rstd), outputs pre-filled with -77."""
    L = _lib()
    M, N = x.shape
    y = torch.full((M, N), -77.0, device=DEV)
    ro = torch.full((M, N), -77.0, device=DEV)
    mean = torch.full((M,), -77.0, device=DEV) if with_mean else None
    rstd = torch.full((M,), -77.0, device=DEV)
    rc = L.lib().fv_add_norm_fwd(
        L.ptr(x), L.i32(L.dtype_code(x.dtype)), L.ptr(res), L.i32(L.dtype_code(res.dtype) if res is not None else 0),
        L.ptr(w), L.ptr(b), L.ptr(rs), L.i32(rows_per_scale), L.ptr(y), L.i32(L.FV_F32), L.ptr(ro), L.i32(L.FV_F32),
        L.ptr(mean), L.ptr(rstd), L.i32(M), L.i32(N), ctypes.c_float(eps), L.i32(rms), L.stream_of(x))
    torch.cuda.synchronize()
    return rc, y, ro, mean, rstd


@pytest.mark.parametrize("N", [192, 768, 260])
@pytest.mark.parametrize("family,kind", [("plain", "rms"), ("plain", "ln"), ("offset", "ln")])
def test_saved_statistics(family, kind, N):
    """mean / rstd as fv_add_norm_fwd leaves them for the backward kernels (the fused ones included)."""
    rms = kind == "rms"
    fails = []
    for B, Ltok in ((9, 7), (257, 1)):
        inp = nc.make_inputs(family, B, Ltok, N, rms)
        ref = nc.reference_of(inp, rms)
        g = lambda t: None if t is None else t.to(DEV).contiguous()
        rc, y, ro, mean, rstd = _c_fwd(g(inp["x"]), g(inp["residual"]), g(inp["w"]), g(inp["b"]), g(inp["row_scale"]),
                                       Ltok, inp["eps"], rms)
        assert rc == 0, _lib().lib().fv_last_error().decode()
        out = {"y": y.cpu(), "r": ro.cpu(), "rstd": rstd.cpu(), "mean": None if rms else mean.cpu()}
        msgs = nc.check_all(out, ref, inp["b"])
        if rms and not torch.equal(mean.cpu(), torch.full((B * Ltok,), -77.0)):
            msgs.append("RMSNorm wrote the mean buffer")
        if msgs:
            fails.append(_ctx(msgs, family=family, N=N, M=B * Ltok, kind=kind))
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------ structure checks, bitwise
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [192, 384, 260, 1028])
def test_repeat_is_bitwise_identical(N, kind):
    rms = kind == "rms"
    for B, Ltok in ((9, 7), (257, 1)):
        inp = nc.make_inputs("plain", B, Ltok, N, rms)
        a, b = run_kernel(inp, rms), run_kernel(inp, rms)
        for k, v in a.items():
            assert v is None or torch.equal(v, b[k]), f"{k} differs between two identical calls (N={N}, M={B * Ltok})"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", [9, 257])
@pytest.mark.parametrize("N", [192, 384, 260])
def test_row_independence(N, M, kind):
    """A row's y, residual_out, dx, dresidual do not depend on which wave slot it lands in: the same rows in reversed
    order (row_scale reversed with them, one sample per row) give the same bits.  dw's summation grouping depends
    on the row order, it is compared under its tolerance."""
    rms = kind == "rms"
    inp = nc.make_inputs("plain", M, 1, N, rms)
    rev = dict(inp)
    for k in ("x", "residual", "dy", "dres", "row_scale"):
        rev[k] = inp[k].flip(0).contiguous()
    a, b = run_kernel(inp, rms), run_kernel(rev, rms)
    for k in ("y", "r", "dx", "dresidual"):
        same = (a[k] == b[k].flip(0)).all(1)
        assert same.all(), f"{k}: rows {(~same).nonzero().flatten()[:8].tolist()} change with their position (N={N}, M={M})"
    ref = nc.reference_of(inp, rms)
    msgs = [m for m in (nc.check_dw(b["dw"], ref), nc.check_db(b["db"], ref) if b["db"] is not None else "") if m]
    assert not msgs, _ctx(msgs, N=N, M=M, kind=kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [192, 260])
def test_direct_weight_gradient_accumulation(N, kind):
    """weight._fv_direct with a preset contiguous fp32 .grad (the flat training state's route): backward adds dw into
    .grad itself and hands autograd no dw, so nothing is added twice."""
    rms = kind == "rms"
    B, Ltok = 9, 7
    inp = nc.make_inputs("plain", B, Ltok, N, rms)
    ref = nc.reference_of(inp, rms)
    from fastvim_amd.layernorm import layer_norm_fn
    sh = lambda t: t.to(DEV).reshape(B, Ltok, N)
    w = torch.nn.Parameter(inp["w"].to(DEV))
    preset = torch.randn(N, generator=torch.Generator().manual_seed(7))
    w.grad = preset.to(DEV).clone()
    w._fv_direct = True
    grad_storage = w.grad.data_ptr()
    b = inp["b"].to(DEV).requires_grad_() if inp["b"] is not None else None
    x, res = sh(inp["x"]).requires_grad_(), sh(inp["residual"]).requires_grad_()
    y, r = layer_norm_fn(x, w, b, residual=res, eps=inp["eps"], prenorm=True, residual_in_fp32=True,
                         is_rms_norm=rms, row_scale=inp["row_scale"].to(DEV))
    torch.autograd.backward((y, r), (sh(inp["dy"]), sh(inp["dres"])))
    assert w.grad.data_ptr() == grad_storage, ".grad was replaced, not accumulated into"
    want = ref["dw"] + preset.double()
    # one fp32 rounding of preset + dw on top of the dw bound
    msg = nc.check_dw(w.grad.cpu(), dict(ref, dw=want), extra=2.0 ** -24 * want.abs())
    assert not msg, _ctx([msg], N=N, kind=kind)
    assert not nc.check_dx(x.grad.cpu().reshape(-1, N), ref)


# ------------------------------------------------------------------------------------------------ host-side refusals
@pytest.mark.parametrize("N", [30, 2052])
def test_unsupported_width_is_refused_before_any_launch(N):
    """Argument checks of the C entry points (FV_CHECK before the launch): nothing is written."""
    from fastvim_amd.layernorm import layer_norm_fn
    L = _lib()
    M = 6
    x = torch.randn(2, 3, N, device=DEV)
    w = torch.ones(N, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 4 and <= 2048"):
        layer_norm_fn(x, w, None, is_rms_norm=True)
    rc, y, ro, mean, rstd = _c_fwd(x.reshape(M, N), None, w, None, None, 1, 1e-5, 1)
    assert rc != 0
    msg = L.lib().fv_last_error().decode()
    assert "2048" in msg and str(N) in msg, msg
    for t in (y, ro, mean, rstd):
        assert (t == -77.0).all(), "a refused call wrote to an output"
    dx = torch.full((M, N), -77.0, device=DEV)
    pw = torch.full((L.lib().fv_add_norm_blocks(L.i32(M)), N), -77.0, device=DEV)
    rstd_in = torch.ones(M, device=DEV)
    dy = torch.randn(M, N, device=DEV)
    rc = L.lib().fv_add_norm_bwd(L.ptr(dy), L.i32(L.FV_F32), L.ptr(None), L.i32(0), L.ptr(x), L.i32(L.FV_F32), L.ptr(w),
                                 L.ptr(None), L.ptr(rstd_in), L.ptr(None), L.i32(1), L.ptr(dx), L.i32(L.FV_F32),
                                 L.ptr(None), L.i32(0), L.ptr(pw), L.ptr(None), L.i32(M), L.i32(N), L.i32(1),
                                 L.stream_of(dy))
    torch.cuda.synchronize()
    assert rc != 0
    msg = L.lib().fv_last_error().decode()
    assert "2048" in msg and str(N) in msg, msg
    assert (dx == -77.0).all() and (pw == -77.0).all(), "a refused call wrote to an output"


def test_row_scale_length_must_divide_the_rows():
    from fastvim_amd.layernorm import layer_norm_fn
    x = torch.randn(3, 5, 192, device=DEV)
    w = torch.ones(192, device=DEV)
    for n in (2, 4, 7, 16):
        with pytest.raises(RuntimeError, match="row_scale"):
            layer_norm_fn(x, w, None, is_rms_norm=True, row_scale=torch.ones(n, device=DEV))
    y = layer_norm_fn(x, w, None, is_rms_norm=True, row_scale=torch.ones(5, device=DEV))     # 15 rows, 5 samples of 3
    assert torch.isfinite(y).all()


def test_layernorm_without_mean_buffer_is_refused():
    L = _lib()
    M, N = 6, 192
    x, w, b = torch.randn(M, N, device=DEV), torch.ones(N, device=DEV), torch.zeros(N, device=DEV)
    rc, y, ro, mean, rstd = _c_fwd(x, None, w, b, None, 1, 1e-5, 0, with_mean=False)
    assert rc != 0
    assert "mean" in L.lib().fv_last_error().decode()
    for t in (y, ro, rstd):
        assert (t == -77.0).all(), "a refused call wrote to an output"
    dx = torch.full((M, N), -77.0, device=DEV)
    pw = torch.full((L.lib().fv_add_norm_blocks(L.i32(M)), N), -77.0, device=DEV)
    rstd_in = torch.ones(M, device=DEV)
    rc = L.lib().fv_add_norm_bwd(L.ptr(x), L.i32(L.FV_F32), L.ptr(None), L.i32(0), L.ptr(x), L.i32(L.FV_F32), L.ptr(w),
                                 L.ptr(None), L.ptr(rstd_in), L.ptr(None), L.i32(1), L.ptr(dx), L.i32(L.FV_F32),
                                 L.ptr(None), L.i32(0), L.ptr(pw), L.ptr(None), L.i32(M), L.i32(N), L.i32(0),
                                 L.stream_of(x))
    torch.cuda.synchronize()
    assert rc != 0
    assert "mean" in L.lib().fv_last_error().decode()
    assert (dx == -77.0).all() and (pw == -77.0).all(), "a refused call wrote to an output"
