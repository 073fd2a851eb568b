"""Float64 references and derived bounds for the fused projection + norm launches, stage by stage.

Plain helpers (no fixtures, nothing here imports ``fastvim_amd``) shared by ``test_fused_proj_ref_cpu.py`` (which pins
them to ``F.linear`` + ``oracle.fused_add_norm_oracle`` and to autograd, and shows that every comparator can fail) and
``test_fused_proj_gpu.py`` (which holds ``fv_gemm_bf16_addnorm2``, ``fv_gemm_bf16_dgrad_addnorm_bwd2``,
``fv_mixer_combine_out_proj_addnorm(_pk)``, ``fv_mixer_conv_pool_bwd_dgrad(_pk)`` and ``fv_gemm_bf16_rowbias`` to them).

The launches compute, per row of M (include/fastvim_hip.h):

  forward    h = bf16_round(A W);  r = residual + s * h (fp32);  rstd = rsqrt(mean_n r^2 + eps);  y = bf16(r rstd w)
  backward   dy = bf16_round(A W);  xhat = r rstd;  dres_in = rstd (dy w - xhat mean_n(dy w xhat)) + dres_out (fp32);
             dx = bf16(s dres_in);  pw[workgroup] = sum over the workgroup's rows of dy xhat
  2nd phase  C2 = bf16(T W2) with T = the bf16 y (forward) or dx (backward) the launch has just written, K = 192

with ``s`` the per-sample DropPath scale ``row_scale[row // rows_per_scale]`` (1 where absent).  ``W`` is handed to the
helpers as (K, N) whatever its storage.

Stage rule (the chaining rule of ``test_mixer_families_gpu.py``): a stage's reference is computed from the launch's inputs
and from outputs of EARLIER stages that the test has just verified -- the norm stage from the stored ``res_out``, the
second phase from the stored ``y`` / ``dx`` -- so a failure names one stage of one launch.

Bounds -- none measured from the kernels.  ``u = 2**-24``; R_TOL, Y_TOL, STAT_TOL, GRAD_TOL are ``norm_checks``'.

* product      the kernels accumulate K terms in fp32 and round the sum to bf16 ONCE before the epilogue (the documented
               contract).  ``eps_x = 2**-8 |P64| + K u (|A| @ |W|)``: half a bf16 ulp of the result (relative 2**-8, the
               rounding of the fp32 sum; its second-order part, 2**-8 times the fp32 error, is a thousandth of the second
               term) plus the standard bound ``gamma_K <= K u`` on a K-term fp32 accumulation in any order.
* res_out      ``|res_out - r64| <= R_TOL rowmax|r64| + |s| eps_x``: norm_checks' bound of the fp32 add, plus the product's
               allowance scaled like the product.  s = 0: ``res_out == residual`` bit for bit (fma(h, 0, r) = r).
* rstd, y      norm_checks' own bounds (``check_rstd``, ``check_y``: bf16 ``y``), reference = ``norm_checks.reference``
               (RMSNorm, no bias) of the STORED ``res_out``.
* dres_in      ``GRAD_TOL rowmax|dres64 - dres_out| + rstd (|w| eps_x + |xhat| mean_n(|w xhat| eps_x))``: norm_checks'
               row bound of the fp32 adjoint arithmetic (cond = 1 for RMSNorm; adding dres_out is one rounding, inside
               it) plus the first-order propagation of an error ``e``, ``|e| <= eps_x``, of dy through
               ``rstd (e w - xhat mean_n(e w xhat))``, absolute values taken term by term.
* dx           ``|s|`` times the dres_in bound plus ``2**-8 |dx64|`` (one bf16 store).  s = 0: ``dx == 0`` exactly.
* pw           per workgroup ``GRAD_TOL sum|dy xhat| + sum(eps_x |xhat|)`` over that workgroup's rows: norm_checks' ``dw``
               bound (cond = 1, sm = 0) restricted to the rows, plus the propagated product error.  Compared per
               workgroup row, never after summing: a row missing from one 64-row sum is 1 / 64 of it, from the sum over
               all rows a part in M.
* C2           ``2**-8 |C2_64| + 192 u (|T| @ |W2|)``: eps_x of a K = 192 product whose operands are exact.
* rowbias      ``C = bf16_round(P) + table[m % period]`` in fp32.  The value rounded to bf16 is the kernel's fp32 sum, not
               P64: where P64 lies within the fp32 error of a rounding boundary the two round to different neighbours,
               a whole ulp apart, so the comparison is with ``P64 + table`` under ``eps_x + u |C64|`` (eps_x already holds
               the rounding; u |C| is the fp32 add), and the rounding itself is checked on its own: ``C - table`` must
               lie within ``u |C|`` (that add) of a bf16 value.
"""
import torch

import norm_checks as N

F64 = torch.float64
U = 2.0 ** -24
HALF_ULP = 2.0 ** -8
K2 = 192          # depth of the second GEMM phase (= d_model)
TILE = 64         # rows of a workgroup of the GEMM-fused forms


def d(t):
    return t.detach().to(F64).cpu()


def bf16_round(t):
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def product(A, W_kn, K=None):
    """P64 = A @ W (A (M, K), W (K, N), values as stored) and eps_x (M, N)."""
    A, W_kn = d(A), d(W_kn)
    K = A.shape[1] if K is None else K
    P = A @ W_kn
    return P, HALF_ULP * P.abs() + K * U * (A.abs() @ W_kn.abs())


def row_scales(row_scale, rows_per_scale, M):
    """(M,) float64 scale of every row: row_scale[row // rows_per_scale], ones where absent."""
    if row_scale is None:
        return torch.ones(M, dtype=F64)
    return d(row_scale).reshape(-1)[torch.arange(M) // rows_per_scale]


def xcd_tile_of_block(block, nblocks):
    """Row tile that hardware workgroup ``block`` of an ``nblocks``-workgroup launch of the GEMM-fused forms owns (the
    XCD-aware remap of csrc/gemm_mfma.hip: workgroup b runs on XCD b % 8; each XCD gets a run of consecutive tiles).  The
    backward form writes pw row ``block``."""
    q8, r8 = divmod(nblocks, 8)
    xcd, j = block % 8, block // 8
    return (xcd * (q8 + 1) if xcd < r8 else r8 * (q8 + 1) + (xcd - r8) * q8) + j


def gemm_pw_rows(M, nblocks):
    """Rows of every pw row of the GEMM-fused backward form: a list of ``nblocks`` long tensors."""
    out = []
    for b in range(nblocks):
        t = xcd_tile_of_block(b, nblocks)
        out.append(torch.arange(t * TILE, min(M, (t + 1) * TILE)))
    return out


def pooling_tile_rows(B, rows, cols, transposed):
    """Memory tokens (rows of M) of every workgroup of the two mixer producer launches: workgroup ``b * ceil(rows / 4) + t``
    owns pooling rows 4 t .. 4 t + 3 of image b."""
    s_i, s_j = (1, rows) if transposed else (cols, 1)
    out = []
    for b in range(B):
        for i0 in range(0, rows, 4):
            i = torch.arange(i0, min(rows, i0 + 4)).view(-1, 1)
            j = torch.arange(cols).view(1, -1)
            out.append((b * rows * cols + i * s_i + j * s_j).reshape(-1))
    return out


# ------------------------------------------------------------------------------------------------ comparators
class Report:
    """Collects failures (messages) and the worst err / bound ratio per output name."""

    def __init__(self):
        self.msgs, self.ratio = [], {}

    def close(self, what, got, ref, bound):
        got, ref, bound = d(got), d(ref), d(bound)
        assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
        g2, r2, b2 = (t.reshape(t.shape[0], -1) if t.dim() else t.reshape(1, 1) for t in (got, ref, bound))
        err = (g2 - r2).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / b2)        # 0 / 0 is inside the bound
        ratio = torch.nan_to_num(ratio, nan=float("inf"))
        worst = ratio.max().item() if ratio.numel() else 0.0
        self.ratio[what] = max(self.ratio.get(what, 0.0), worst)
        m = N._worst(err, b2, what)
        if m:
            self.msgs.append(m)
        return not m

    def note(self, msg):
        if msg:
            self.msgs.append(msg)

    def __bool__(self):
        return not self.msgs


def check_forward(rep, P, eps_x, residual, srow, w, eps, res_out, rstd, y, tag=""):
    """Forward epilogue: res_out against ``residual + s P64``; rstd and the bf16 y against norm_checks.reference of the
    stored res_out."""
    r64 = d(residual) + srow[:, None] * P
    bound = N.R_TOL * r64.abs().amax(1, keepdim=True) + srow.abs()[:, None] * eps_x
    ok = rep.close(tag + "res_out", res_out, r64, bound)
    z = srow == 0
    if z.any() and not torch.equal(d(res_out)[z], d(residual)[z]):
        rep.note(tag + "res_out: a row with scale 0 differs from its residual")
    ref = N.reference(res_out.detach().cpu(), w.detach().cpu(), None, None, None, eps, True, None, None)
    rep.close(tag + "rstd", rstd, ref["rstd"], N.STAT_TOL * ref["cond"] * ref["rstd"])
    assert y.dtype == torch.bfloat16
    y64 = ref["y"]
    rep.close(tag + "y", y, y64, N.Y_TOL * ref["cond"][:, None] * y64.abs().amax(1, keepdim=True) + HALF_ULP * y64.abs())
    return ok


def backward_ref(P, eps_x, r, rstd, w, dres_out, srow):
    """Closed-form fp64 adjoint and its bounds: dict with dres, dx, b_dres, b_dx (M, N), t = dy * xhat, t_abs, t_eps
    (M, N: the addends of pw, their magnitudes and their propagated product error)."""
    r, rstd, w = d(r), d(rstd).reshape(-1, 1), d(w)
    xhat = r * rstd
    dyw = P * w
    core = rstd * (dyw - xhat * (dyw * xhat).mean(1, keepdim=True))
    dres = core if dres_out is None else core + d(dres_out)
    dx = srow[:, None] * dres
    prop = rstd * (w.abs() * eps_x + xhat.abs() * ((w * xhat).abs() * eps_x).mean(1, keepdim=True))
    b_dres = N.GRAD_TOL * core.abs().amax(1, keepdim=True) + prop
    b_dx = srow.abs()[:, None] * b_dres + HALF_ULP * dx.abs()
    t = P * xhat
    return dict(dres=dres, dx=dx, b_dres=b_dres, b_dx=b_dx, t=t, t_abs=t.abs(), t_eps=eps_x * xhat.abs())


def check_backward(rep, P, eps_x, r, rstd, w, dres_out, srow, dres_in, dx, pw, pw_rows, tag=""):
    """Backward epilogue: dres_in, bf16 dx, and every pw row against the sum over ITS rows (``pw_rows``: one long tensor of
    row indices per pw row)."""
    b = backward_ref(P, eps_x, r, rstd, w, dres_out, srow)
    rep.close(tag + "dres_in", dres_in, b["dres"], b["b_dres"])
    assert dx.dtype == torch.bfloat16
    rep.close(tag + "dx", dx, b["dx"], b["b_dx"])
    z = srow == 0
    if z.any() and bool((d(dx)[z] != 0).any()):
        rep.note(tag + "dx: a row with scale 0 is not zero")
    if len(pw_rows) != pw.shape[0]:
        rep.note(f"{tag}pw: {pw.shape[0]} rows for {len(pw_rows)} workgroups")
        return b
    ref = torch.stack([b["t"][i].sum(0) for i in pw_rows])
    bound = torch.stack([N.GRAD_TOL * b["t_abs"][i].sum(0) + b["t_eps"][i].sum(0) for i in pw_rows])
    rep.close(tag + "pw", pw, ref, bound)
    return b


def check_second(rep, T, W2_kn, C2, tag=""):
    """Second GEMM phase: C2 (bf16) against T @ W2, T the stored bf16 tile (M, 192), W2 (192, N2)."""
    assert T.dtype == torch.bfloat16 and C2.dtype == torch.bfloat16
    T, W2_kn = d(T), d(W2_kn)
    C64 = T @ W2_kn
    return rep.close(tag + "C2", C2, C64, HALF_ULP * C64.abs() + K2 * U * (T.abs() @ W2_kn.abs()))


def check_rowbias(rep, P, eps_x, table, C, tag=""):
    """fv_gemm_bf16_rowbias: C (fp32) against P64 + table[m % period], and C - table against the nearest bf16 value."""
    M = P.shape[0]
    t = d(table)[torch.arange(M) % table.shape[0]]
    C64 = P + t
    rep.close(tag + "C", C, C64, eps_x + U * C64.abs())
    h = d(C) - t
    rep.close(tag + "C - table is bf16", h, bf16_round(h), U * d(C).abs())


# ------------------------------------------------------------------------------------------------ fp32 emulation
def emulate_forward(A, W_kn, residual, srow, w, eps):
    """A plain fp32 evaluation of the forward launch on the CPU: fp32 matmul of the bf16-valued operands, ``.bfloat16()`` at
    the documented point, fp32 epilogue.  Returns res_out, rstd (fp32), y (bf16)."""
    h = (A.float() @ W_kn.float()).bfloat16().float()
    r = residual.float() + srow.float()[:, None] * h
    rstd = torch.rsqrt(r.square().mean(1) + eps)
    return r, rstd, (r * rstd[:, None] * w.float()).bfloat16()


def emulate_backward(A, W_kn, r, rstd, w, dres_out, srow, pw_rows):
    """The same for the backward launch: dres_in (fp32), dx (bf16), pw (len(pw_rows), N) fp32."""
    dy = (A.float() @ W_kn.float()).bfloat16().float()
    xhat = r.float() * rstd.float()[:, None]
    dyw = dy * w.float()
    dres = rstd.float()[:, None] * (dyw - xhat * (dyw * xhat).mean(1, keepdim=True))
    if dres_out is not None:
        dres = dres + dres_out.float()
    dx = (dres * srow.float()[:, None]).bfloat16()
    pw = torch.stack([(dy * xhat)[i].sum(0) for i in pw_rows])
    return dres, dx, pw
