"""The comparators of ``norm_checks.py`` must be able to fail (no GPU needed).

A correct fp32 two-pass emulation of the fused add + norm forward and backward (plain torch, the arithmetic of
``csrc/norm.hip`` without its lane layout) passes every comparator on every input family with a margin; the same
emulation with one deliberate defect fails the comparator named for it.  This is what makes the sensitivity of
``test_norm_edges_gpu.py`` checkable on a machine without a GPU.
"""
import pytest
import torch

import norm_checks as nc

F32, BF16 = torch.float32, torch.bfloat16
WIDTHS = (4, 32, 192, 260, 768, 1028, 2048)


def _store(t, dt, truncate=False):
    if dt == F32:
        return t
    if truncate:           # drop the low 16 bits instead of rounding to nearest even
        return (t.contiguous().view(torch.int32) & -65536).view(F32).to(BF16)
    return t.to(BF16)


def emulate(inp, rms, *, res_dt=F32, y_dt=None, defect=None, dy=True, dres=True):
    """fp32 two-pass forward and backward; returns the kernel's outputs (y, r, mean, rstd, dx, dresidual, dw, db).
    ``defect`` switches one deliberate error on."""
    x, res, w, b = inp["x"], inp["residual"], inp["w"], inp["b"]
    M, N = x.shape
    y_dt = y_dt or x.dtype
    sc = nc.rows_scale(inp["row_scale"], M)
    xf = x.float()
    if res is not None:
        # the kernel's fmaf(x, scale, residual): one rounding of the exact value (the fp64 product of two fp32 is exact)
        r = (xf.double() * sc.double()[:, None] + res.double()).float() if sc is not None else xf + res.float()
    else:
        r = xf * sc[:, None] if sc is not None else xf
    r_st = _store(r, res_dt)
    cols = N - 4 if defect == "stats_skip_last4" else N
    if rms:
        mean = torch.zeros(M)
    elif defect == "one_pass":
        mean = r.sum(1) / N
    else:
        mean = r[:, :cols].sum(1) / N
    if defect == "one_pass":
        var = (r * r).sum(1) / N - mean * mean
    else:
        d = r[:, :cols] - mean[:, None]
        var = (d * d).sum(1) / N
    rstd = torch.rsqrt(var + inp["eps"])
    y = (r - mean[:, None]) * rstd[:, None] * w
    if b is not None:
        y = y + b
    y = _store(y, y_dt, truncate=(defect == "bf16_truncate"))
    # backward: reads the STORED residual_out and the saved statistics, like the kernel
    rb = r_st.float()
    dyf = inp["dy"].float() if dy else torch.zeros(M, N)
    xh = (rb - mean[:, None]) * rstd[:, None]
    dxh = dyf * w
    c2 = (dxh * xh).sum(1, keepdim=True) / N
    c1 = torch.zeros(M, 1) if (rms or defect == "drop_c1") else dxh.sum(1, keepdim=True) / N
    dr = rstd[:, None] * (dxh - c1 - xh * c2)
    if dres:
        dr = dr + inp["dres"].float()
    sc_b = sc
    if defect == "scale_index" and sc is not None:
        rps = M // inp["row_scale"].numel()
        sc_b = inp["row_scale"][torch.arange(M) // (rps + 1)]
    dx = dr if (sc_b is None or defect == "dx_no_scale") else dr * sc_b[:, None]
    contrib = dyf * xh
    dw = contrib.sum(0)
    if defect == "dw_skip_last":
        dw = contrib[:-1].sum(0)
    elif defect == "dw_double_last":
        dw = contrib.sum(0) + contrib[-1]
    out = {"y": y, "r": r_st, "mean": None if rms else mean, "rstd": rstd,
           "dx": _store(dx, x.dtype), "dresidual": _store(dr, res.dtype) if res is not None else None,
           "dw": dw, "db": dyf.sum(0) if b is not None else None}
    return out


def _cases():
    for family in nc.FAMILIES:
        for rms in (True, False):
            if nc.family_applies(family, rms):
                yield family, rms


@pytest.mark.parametrize("family,rms", list(_cases()))
@pytest.mark.parametrize("N", WIDTHS)
def test_correct_fp32_emulation_passes_every_comparator(family, rms, N):
    """The reference alone stays within the bound -- and with a margin: every error is asserted at a THIRD of its
    bound (the comparators are re-run on errors scaled by 3), so a correct fp32 kernel has room."""
    for B, Ltok in ((1, 1), (2, 1), (3, 1), (9, 7), (257, 1)):
        inp = nc.make_inputs(family, B, Ltok, N, rms)
        ref = nc.reference_of(inp, rms)
        out = emulate(inp, rms)
        msgs = nc.check_all(out, ref, inp["b"])
        assert not msgs, f"{family} rms={rms} N={N} M={B * Ltok}: " + "; ".join(msgs)
        # margin: out3 = ref + 3 * (out - ref) must still pass
        out3 = {k: (ref[k] + 3 * (v.double() - ref[k])).float() for k, v in out.items() if v is not None}
        msgs = nc.check_all(out3, ref, inp["b"])
        assert not msgs, f"margin below 3x, {family} rms={rms} N={N} M={B * Ltok}: " + "; ".join(msgs)


@pytest.mark.parametrize("rms", [True, False])
@pytest.mark.parametrize("N", [192, 260])
def test_correct_bf16_emulation_passes_every_comparator(rms, N):
    """bf16 x / y / dx with an fp32 residual, and the bf16-residual form (residual_out stored in bf16, the backward
    reads the rounded tensor): inside the bf16 bounds, the latter only with its one derived allowance."""
    for family in ("plain", "scale0"):
        inp = nc.make_inputs(family, 9, 7, N, rms, xdt=BF16)
        ref = nc.reference_of(inp, rms)
        msgs = nc.check_all(emulate(inp, rms), ref, inp["b"])
        assert not msgs, f"{family} bf16 x: " + "; ".join(msgs)
        inp = nc.make_inputs(family, 9, 7, N, rms, xdt=BF16, res_dt=BF16)
        ref = nc.reference_of(inp, rms)
        out = emulate(inp, rms, res_dt=BF16)
        msgs = nc.check_all(out, ref, inp["b"], stored_r_bf16=True)
        assert not msgs, f"{family} bf16 residual: " + "; ".join(msgs)
    # out_dtype = bf16 on fp32 x: y bf16, gradients fp32
    inp = nc.make_inputs("plain", 9, 7, N, rms)
    inp["dy"] = inp["dy"].to(BF16)
    ref = nc.reference_of(inp, rms)
    out = emulate(inp, rms, y_dt=BF16)
    assert out["y"].dtype == BF16 and out["dx"].dtype == F32
    assert not nc.check_all(out, ref, inp["b"])


# defect -> (family, rms, comparator that must fail)
DEFECTS = {
    "one_pass": ("offset", False, "y"),
    "dw_skip_last": ("plain", True, "dw"),
    "dw_double_last": ("plain", True, "dw"),
    "scale_index": ("plain", True, "dx"),
    "dx_no_scale": ("plain", True, "dx"),
    "drop_c1": ("plain", False, "dx"),
    "bf16_truncate": ("plain", True, "y"),
    "stats_skip_last4": ("plain", True, "y"),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
@pytest.mark.parametrize("N", [192, 260, 1028])
def test_wrong_emulation_fails_its_comparator(defect, N):
    family, rms, key = DEFECTS[defect]
    B, Ltok = 9, 7
    inp = nc.make_inputs(family, B, Ltok, N, rms)
    y_dt = None
    if defect == "bf16_truncate":
        y_dt = BF16
        inp["dy"] = inp["dy"].to(BF16)
    if defect in ("dw_skip_last", "dw_double_last"):
        # few-hot upstream gradient: dy lives on the first and the last row only, so one missing or doubled row is an
        # error of order 1 in the units of the bound (sum_rows |dy * xhat| has two addends)
        hot = torch.zeros(B * Ltok, 1)
        hot[0] = hot[-1] = 1
        inp["dy"] = inp["dy"] * hot
    ref = nc.reference_of(inp, rms)
    good = emulate(inp, rms, y_dt=y_dt)
    assert not nc.check_all(good, ref, inp["b"]), "the correct emulation must pass on the same inputs"
    bad = emulate(inp, rms, y_dt=y_dt, defect=defect)
    check = {"y": lambda o: nc.check_y(o["y"], ref, inp["b"]), "dx": lambda o: nc.check_dx(o["dx"], ref),
             "dw": lambda o: nc.check_dw(o["dw"], ref)}[key]
    msg = check(bad)
    assert msg, f"{defect} at N={N} was not caught by check_{key}"
    assert msg.startswith(key)
    if defect == "one_pass":
        assert nc.check_rstd(bad["rstd"], ref), "one-pass variance must fail the rstd check too"
    if defect == "stats_skip_last4":
        assert nc.check_rstd(bad["rstd"], ref)


def test_dense_dw_would_hide_a_doubled_last_row_less_well():
    """Why the GPU tests use few-hot gradients: with a dense dy over 257 rows a doubled last row moves dw by about
    1/257 of sum|dy * xhat| -- still caught by the 2e-5 bound, but under the old max-of-tensor tolerance floored at
    1.0 the same error at 9 rows and small dy is not.  The row-wise bound has no floor."""
    inp = nc.make_inputs("plain", 9, 1, 192, True)
    inp["dy"] = inp["dy"] * 1e-6          # small upstream gradient: the old floor would turn into an absolute 2e-5
    ref = nc.reference_of(inp, True)
    bad = emulate(inp, True, defect="dw_double_last")
    old_style = (bad["dw"].double() - ref["dw"]).abs().max().item() <= 2e-5 * max(1.0, ref["dw"].abs().max().item())
    assert old_style, "premise: the floored tensor-wide tolerance lets this through"
    assert nc.check_dw(bad["dw"], ref)


def test_dw_bound_needs_its_absolute_term_at_few_rows():
    """Why check_dw carries ``sum|dy| * (cond - 1)``: without it the correct fp32 emulation of LayerNorm breaks the
    bound ``2e-5 * cond * sum|dy * xhat|`` at M = 1 in some column where |xhat| is small (derivation in norm_checks.py)."""
    broken = 0
    for N in WIDTHS:
        for seed in range(8):
            inp = nc.make_inputs("plain", 1, 1, N, False, seed=seed)
            ref = nc.reference_of(inp, False)
            out = emulate(inp, False)
            assert not nc.check_dw(out["dw"], ref), (N, seed)
            broken += bool(nc.check_dw(out["dw"], dict(ref, sm=torch.zeros(N, dtype=torch.float64))))
    assert broken > 0, "premise gone: the relative-only bound now holds for the fp32 emulation; drop the absolute term"


def test_zero_reference_rows_must_be_exactly_zero():
    inp = nc.make_inputs("scale0", 9, 7, 192, True)
    ref = nc.reference_of(inp, True)
    out = emulate(inp, True)
    assert not nc.check_dx(out["dx"], ref)
    rows = slice((9 // 2) * 7, (9 // 2 + 1) * 7)
    assert ref["dx"][rows].abs().max().item() == 0.0
    out["dx"][rows.start, 5] = 1e-30
    msg = nc.check_dx(out["dx"], ref)
    assert msg and f"row {rows.start} col 5" in msg


def test_nan_is_a_failure():
    inp = nc.make_inputs("plain", 3, 3, 32, True)
    ref = nc.reference_of(inp, True)
    out = emulate(inp, True)
    out["y"][4, 7] = float("nan")
    assert "row 4 col 7" in nc.check_y(out["y"], ref, None)


def test_oracle_out_dtype_argument():
    from oracle import fused_add_norm_oracle
    x, w, res = torch.randn(2, 5, 32), torch.ones(32), torch.randn(2, 5, 32)
    y0, r0 = fused_add_norm_oracle(x, w, None, res, 1e-5, True, True, True)
    y1, r1 = fused_add_norm_oracle(x, w, None, res, 1e-5, True, True, True, out_dtype=BF16)
    assert y0.dtype == F32 and y1.dtype == BF16 and r1.dtype == F32
    assert torch.equal(r0, r1)
    y64 = fused_add_norm_oracle(x, w, None, res, 1e-5, False, True, True, out_dtype=torch.float64)
    assert torch.equal(y1, y64.to(BF16)), "the folded cast rounds the unrounded result once"
