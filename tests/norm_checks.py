"""Row-wise comparison of the fused add + RMSNorm / LayerNorm op with an unrounded fp64 reference.

Plain helpers (no fixtures) shared by ``test_norm_checks_cpu.py`` (the checks must be able to fail) and
``test_norm_edges_gpu.py`` (the HIP kernels of ``csrc/norm.hip``).  Nothing here imports ``fastvim_amd``.

Every tensor is handled as ``(M, N)`` rows; ``row_scale`` is the per-sample DropPath scale ``(B,)`` with
``M % B == 0``, sample ``i`` owning rows ``i*M/B .. (i+1)*M/B - 1``.

Bounds.  ``u = 2**-24``.  Per row ``cond = 1 + |mean| * rstd`` (1 for RMSNorm): ``r - mean`` carries an absolute
error of about ``u * |mean|`` and is then multiplied by ``rstd``, so a LayerNorm row that sits ``k`` standard
deviations off zero loses a factor ``1 + k`` of fp32's relative precision.  ``cond`` is derived, not tuned.

* fp32 ``y``             ``|y - y64| <= 3e-6 * (cond * rowmax|y64 - b| + max|b|)``
* ``residual_out``       ``<= 1e-6 * rowmax|r64|``                      (bf16 storage: ``+ 2**-8 * |r64|``)
* ``rstd``               ``<= 3e-6 * cond * rstd64``
* ``mean``               ``<= 3e-6 * (|mean64| + 1 / rstd64)``
* fp32 ``dx, dresidual`` ``<= 2e-5 * cond * rowmax|ref|``     (a row whose reference is all zero must be all zero)
* ``dw``                 per column ``<= 2e-5 * (max_rows(cond) * sum_rows|dy * xhat| + sum_rows|dy| * (cond - 1))``
* ``db``                 per column ``<= 2e-5 * max_rows(cond) * sum_rows|dy|``
* bf16 ``y, dx, dresidual``  the fp32 term ``+ 2**-8 * |ref64|``: round-to-nearest into 8 significant bits is off
  by at most half an ulp, at most ``2**-8`` relative (a truncating store reaches ``2**-7`` and fails).
* ``stored_r_bf16=True`` (bf16 residual form only: the kernel stores ``residual_out`` in bf16 and the backward
  reads that rounded tensor while ``mean`` / ``rstd`` come from the unrounded sum, as the reference's Triton
  kernel does): ``dx`` / ``dresidual`` get ``+ 2**-8 * rowmax|ref|`` and ``dw`` gets
  ``+ 2**-8 * (sum_rows|dy * xhat| + sum_rows|dy| * (cond - 1))``, an allowance for that one storage rounding,
  used nowhere else.

The second addend of the ``dw`` bound is the same derivation as ``cond``, kept absolute: the error ``u * |mean|`` of
``r - mean`` times ``rstd`` is an ABSOLUTE error ``u * (cond - 1)`` of ``xhat``.  Row-wise it hides inside
``cond * rowmax`` (``rowmax|xhat| >= 1``); per column it does not when the sum has few addends and ``|xhat|`` happens
to be small there: at M = 1 a LayerNorm column with ``|xhat| = 1e-4`` (one element in ten thousand) has
``2e-5 * cond * |dy * xhat| = 2e-9 |dy|`` while a correct fp32 evaluation is off by ``u * |mean| * rstd |dy|``, about
``4e-9 |dy|`` at N = 192 (``|mean| * rstd`` is about ``1 / sqrt(N)`` for zero-mean data).  The plain fp32 emulation of
``test_norm_checks_cpu.py`` shows it at M = 1 .. 3 (``test_dw_bound_needs_its_absolute_term_at_few_rows``).  The term
is 0 for RMSNorm and of relative size ``(cond - 1) / |xhat|`` otherwise: a missing or doubled row is still an error of
order 1 in these units.

3e-6 / 1e-6 / 2e-5 are the fp32 numbers of ``test_norm_gpu.py::test_norm_fwd_bwd_vs_oracle`` applied per row
instead of per tensor; there is no ``max(1.0, ...)`` floor anywhere.  A plain fp32 two-pass evaluation of the
same formulas stays 6x or more below them (``test_norm_checks_cpu.py`` keeps that in the suite).
"""
import torch

F64 = torch.float64
BF16_HALF_ULP = 2.0 ** -8
Y_TOL, R_TOL, STAT_TOL, GRAD_TOL = 3e-6, 1e-6, 3e-6, 2e-5


def rows_scale(row_scale, M):
    """(B,) per-sample scale -> (M,) per-row scale (None stays None)."""
    if row_scale is None:
        return None
    B = row_scale.numel()
    assert M % B == 0
    return row_scale.reshape(-1).repeat_interleave(M // B)


def reference(x, w, b, residual, row_scale, eps, rms, dy, dres):
    """Unrounded fp64 forward and backward of the operation from its definition (``oracle/norm.py``'s formula,
    gradients by fp64 autograd).  ``x, residual, dy, dres`` are (M, N) (any float dtype; ``residual``, ``dy``,
    ``dres`` may be None = absent / zero), ``w, b`` (N,), ``row_scale`` (B,) or None.  Runs on the tensors' device.
    Returns a dict of fp64 tensors: y, r, mean, rstd, cond (M,), dx, dresidual, dw, db, sw = sum_rows|dy * xhat|,
    sb = sum_rows|dy|, sm = sum_rows|dy| * (cond - 1) (N,)."""
    M, N = x.shape
    xf = x.detach().to(F64).requires_grad_()
    wf = w.detach().to(F64).requires_grad_()
    bf = b.detach().to(F64).requires_grad_() if b is not None else None
    rf = residual.detach().to(F64).requires_grad_() if residual is not None else None
    sc = rows_scale(row_scale, M)
    xs = xf if sc is None else xf * sc.to(F64)[:, None]
    r = xs if rf is None else xs + rf
    r.retain_grad()
    if rms:
        mean = torch.zeros(M, dtype=F64, device=x.device)
        rstd = torch.rsqrt(r.square().mean(-1) + eps)
        xhat = r * rstd[:, None]
    else:
        mean = r.mean(-1)
        rstd = torch.rsqrt((r - mean[:, None]).square().mean(-1) + eps)
        xhat = (r - mean[:, None]) * rstd[:, None]
    y = xhat * wf
    if bf is not None:
        y = y + bf
    dyf = torch.zeros_like(y) if dy is None else dy.detach().to(F64)
    loss = (y * dyf).sum()
    if dres is not None:
        loss = loss + (r * dres.detach().to(F64)).sum()
    loss.backward()
    xh = xhat.detach()
    out = {
        "y": y.detach(), "r": r.detach(), "mean": mean.detach(), "rstd": rstd.detach(),
        "cond": (1 + mean.abs() * rstd).detach(),
        "dx": xf.grad, "dresidual": rf.grad if rf is not None else None,
        "dw": wf.grad, "db": bf.grad if bf is not None else None,
        "sw": (dyf * xh).abs().sum(0), "sb": dyf.abs().sum(0),
    }
    out["sm"] = (dyf.abs() * (out["cond"] - 1)[:, None]).sum(0)
    return out


def _worst(err, bound, what):
    """'' when err <= bound everywhere, else a message naming the worst row (and column)."""
    err = err.reshape(err.shape[0], -1)
    bound = torch.as_tensor(bound, dtype=F64, device=err.device)
    bound = bound.reshape(bound.shape[0], -1).expand_as(err)
    bad = ~(err <= bound)          # NaN in err counts as bad
    if not bad.any():
        return ""
    excess = torch.where(bad, err - bound, torch.full_like(err, -1.0))
    excess = torch.nan_to_num(excess, nan=float("inf"))
    i = int(excess.argmax())
    row, col = divmod(i, err.shape[1])
    return (f"{what}: {int(bad.sum())} element(s) over the bound in {int(bad.any(1).sum())} row(s); worst at row {row} "
            f"col {col}: err {err[row, col].item():.3e} > bound {bound[row, col].item():.3e}")


def _d(t):
    return t.detach().to(F64)


def check_y(y, ref, b=None):
    y64 = ref["y"]
    b64 = _d(b).to(y64.device) if b is not None else None
    core = y64 if b64 is None else y64 - b64
    bound = Y_TOL * (ref["cond"][:, None] * core.abs().amax(1, keepdim=True) + (b64.abs().max() if b64 is not None else 0.0))
    what = "y"
    if y.dtype == torch.bfloat16:
        bound, what = bound + BF16_HALF_ULP * y64.abs(), "y(bf16)"
    else:
        assert y.dtype == torch.float32
    return _worst((_d(y) - y64).abs(), bound, what)


def check_r(r, ref):
    r64 = ref["r"]
    bound = (R_TOL * r64.abs().amax(1, keepdim=True)).expand_as(r64)
    what = "residual_out"
    if r.dtype == torch.bfloat16:
        bound, what = bound + BF16_HALF_ULP * r64.abs(), "residual_out(bf16)"
    else:
        assert r.dtype == torch.float32
    return _worst((_d(r) - r64).abs(), bound, what)


def check_rstd(rstd, ref):
    return _worst((_d(rstd) - ref["rstd"]).abs()[:, None], (STAT_TOL * ref["cond"] * ref["rstd"])[:, None], "rstd")


def check_mean(mean, ref):
    return _worst((_d(mean) - ref["mean"]).abs()[:, None],
                  (STAT_TOL * (ref["mean"].abs() + 1 / ref["rstd"]))[:, None], "mean")


def _check_row_grad(g, g64, ref, what, stored_r_bf16):
    rmax = g64.abs().amax(1, keepdim=True)
    bound = (GRAD_TOL * ref["cond"][:, None] * rmax).expand_as(g64)
    if stored_r_bf16:
        bound = bound + BF16_HALF_ULP * rmax
    if g.dtype == torch.bfloat16:
        bound, what = bound + BF16_HALF_ULP * g64.abs(), what + "(bf16)"
    else:
        assert g.dtype == torch.float32
    return _worst((_d(g) - g64).abs(), bound, what)


def check_dx(dx, ref, stored_r_bf16=False):
    return _check_row_grad(dx, ref["dx"], ref, "dx", stored_r_bf16)


def check_dresidual(dres, ref, stored_r_bf16=False):
    return _check_row_grad(dres, ref["dresidual"], ref, "dresidual", stored_r_bf16)


def check_dw(dw, ref, stored_r_bf16=False, extra=None):
    """``extra`` (N,): additional absolute allowance per column (the direct-accumulation test's preset rounding)."""
    assert dw.dtype == torch.float32
    bound = GRAD_TOL * (ref["cond"].max() * ref["sw"] + ref["sm"])
    if stored_r_bf16:
        bound = bound + BF16_HALF_ULP * (ref["sw"] + ref["sm"])
    if extra is not None:
        bound = bound + extra
    return _worst((_d(dw) - ref["dw"]).abs()[None, :], bound[None, :], "dw")


def check_db(db, ref):
    assert db.dtype == torch.float32
    return _worst((_d(db) - ref["db"]).abs()[None, :], (GRAD_TOL * ref["cond"].max() * ref["sb"])[None, :], "db")


def check_all(out, ref, b=None, stored_r_bf16=False):
    """Every comparator whose tensor is present in ``out`` (keys y, r, mean, rstd, dx, dresidual, dw, db); returns
    the list of failure messages (empty = all inside their bounds)."""
    msgs = []
    for key, fn in (("y", lambda t: check_y(t, ref, b)), ("r", lambda t: check_r(t, ref)),
                    ("mean", lambda t: check_mean(t, ref)), ("rstd", lambda t: check_rstd(t, ref)),
                    ("dx", lambda t: check_dx(t, ref, stored_r_bf16)),
                    ("dresidual", lambda t: check_dresidual(t, ref, stored_r_bf16)),
                    ("dw", lambda t: check_dw(t, ref, stored_r_bf16)), ("db", lambda t: check_db(t, ref))):
        t = out.get(key)
        if t is not None:
            m = fn(t.reshape(-1, t.shape[-1]) if t.dim() > 1 else t)
            if m:
                msgs.append(m)
    return msgs


# ------------------------------------------------------------------------------------------------ input families
FAMILIES = ("plain", "offset", "scaled", "scaled_eps0", "zero_rows", "scale0", "scale0_nores")


def family_applies(family, rms):
    """offset separates one-pass from two-pass LayerNorm statistics (RMSNorm has no mean to cancel);
    scaled_eps0 is RMSNorm without bias only (with eps = 0 a LayerNorm row has no scale-free bias term)."""
    return {"offset": not rms, "scaled_eps0": rms}.get(family, True)


def make_inputs(family, B, Ltok, N, rms, xdt=torch.float32, res_dt=torch.float32, seed=0, with_scale=True):
    """CPU inputs of one family as a dict: x, residual (M, N), w, b (N,), row_scale (B,), eps, dy, dres (M, N), B.
    ``dy`` is stored in the dtype the kernel receives it in (the dtype of ``y`` = ``xdt``)."""
    g = torch.Generator().manual_seed(1000 * N + 10 * B * Ltok + seed)
    M = B * Ltok
    rn = lambda *s: torch.randn(*s, generator=g)
    x, res = rn(M, N), rn(M, N)
    w = 1 + 0.1 * rn(N)
    b = None if rms or family == "scaled_eps0" else 0.1 * rn(N)
    eps = 1e-5
    pow2 = None
    # B distinct, non-trivial DropPath scales 1 / keep_prob; sample 0 is dropped (scale 0) when there are >= 3 samples
    row_scale = 1.0 / (1.0 - 0.05 * (1 + torch.arange(B, dtype=torch.float32) % 9))
    if B >= 3:
        row_scale[0] = 0.0
    if family == "offset":
        sign = torch.where(torch.arange(M) % 2 == 0, 1.0, -1.0)
        res = res + 1000.0 * sign[:, None]
    elif family in ("scaled", "scaled_eps0"):
        k = torch.randint(-40, 41, (M,), generator=g)
        f = pow2 = torch.pow(torch.tensor(2.0), k.float())[:, None]      # exact powers of two, (M, 1)
        x, res = x * f, res * f
        if family == "scaled_eps0":
            eps = 0.0
    elif family == "zero_rows":
        x[::7] = 0
        res[::7] = 0
    elif family in ("scale0", "scale0_nores"):
        row_scale[B // 2] = 0.0
        if family == "scale0_nores":
            res = None
    x = x.to(xdt)
    if res is not None:
        res = res.to(res_dt)
    dy = rn(M, N).to(xdt)
    dres = rn(M, N).to(res_dt)
    return {"x": x, "residual": res, "w": w, "b": b, "row_scale": row_scale if with_scale else None, "eps": eps,
            "dy": dy, "dres": dres, "B": B, "family": family, "pow2": pow2}


def reference_of(inp, rms, dy=True, dres=True, device=None):
    t = (lambda v: v if (v is None or device is None) else v.to(device))
    return reference(t(inp["x"]), t(inp["w"]), t(inp["b"]), t(inp["residual"]), t(inp["row_scale"]), inp["eps"], rms,
                     t(inp["dy"]) if dy else None, t(inp["dres"]) if dres else None)
