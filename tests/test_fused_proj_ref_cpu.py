"""Pins the float64 references of ``fused_proj_ref.py`` and shows that its comparators can fail.  No GPU.

* The forward composition (product, scaled residual add, RMSNorm) equals ``F.linear`` in float64 followed by
  ``oracle.fused_add_norm_oracle(prenorm=True, is_rms_norm=True, row_scale=...)`` to 1e-12, and the closed-form backward
  equals autograd of that composition to 1e-12: a reference that is itself wrong cannot agree with a wrong kernel.
* A plain fp32 emulation of the launches (``emulate_forward`` / ``emulate_backward``: torch fp32 matmul of bf16-valued
  operands, ``.bfloat16()`` at the documented point, fp32 epilogue) passes every comparator at M = 1 and 200,
  K = 64 .. 1536, plain rows, rows 3 sigma off zero and rows scaled by 30 -- the derived bounds are not too tight for a
  correct evaluation.  Its worst err / bound ratios are 0.70 - 0.99 forward and 0.35 - 0.97 backward: the half-ulp term
  is tight by construction, the fp32 part stays several times under its share.
* On the same data each of six defects fails at least one comparator: a dropped last K tile, a 1 % product error, a
  one-row shift, an omitted ``dres_out``, a ``dres_in`` multiplied by the DropPath scale, and a ``pw`` row with one row
  missing.
"""
import pytest
import torch
import torch.nn.functional as F

import fused_proj_ref as R
import norm_checks as N
from oracle import fused_add_norm_oracle

F64 = torch.float64
EPS = 1e-5
NCOL = 192


def _data(M, K, family, seed=0, B=None):
    g = torch.Generator().manual_seed(7919 * K + 31 * M + seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    A = rn(M, K).bfloat16()
    W = (rn(K, NCOL) * K ** -0.5).bfloat16()
    res = rn(M, NCOL)
    if family == "offset":
        res = res + 3.0 * torch.where(torch.arange(M) % 2 == 0, 1.0, -1.0)[:, None]
    elif family == "scaled":
        res = res * 30.0
    B = B or (4 if M % 4 == 0 else 1)
    rps = M // B
    scale = 1.0 / (1.0 - 0.05 * (1 + torch.arange(B, dtype=torch.float32)))
    if B >= 3:
        scale[1] = 0.0
    w = 1 + 0.1 * rn(NCOL)
    r = res.clone()
    rstd = torch.rsqrt(r.square().mean(1) + EPS)
    dres_out = rn(M, NCOL)
    nb = -(-M // R.TILE)
    return dict(A=A, W=W, res=res, scale=scale, rps=rps, srow=R.row_scales(scale, rps, M), w=w, r=r, rstd=rstd,
                dres_out=dres_out, pw_rows=R.gemm_pw_rows(M, nb), M=M, K=K)


# ------------------------------------------------------------------------------------------------ pins
@pytest.mark.parametrize("M,K", [(1, 64), (12, 128), (200, 384)])
def test_forward_composition_equals_linear_then_oracle(M, K):
    t = _data(M, K, "plain")
    P, _ = R.product(t["A"], t["W"])
    r64 = R.d(t["res"]) + t["srow"][:, None] * P
    ref = N.reference(r64, t["w"], None, None, None, EPS, True, None, None)
    h = F.linear(t["A"].double(), t["W"].double().t())
    B = t["scale"].numel()
    y, r = fused_add_norm_oracle(h.view(B, M // B, NCOL), t["w"].double(), None, t["res"].double().view(B, M // B, NCOL), eps=EPS,
                                 prenorm=True, is_rms_norm=True, row_scale=t["scale"].double())
    assert (r.reshape(M, NCOL) - r64).abs().max().item() <= 1e-12
    assert (y.reshape(M, NCOL) - ref["y"]).abs().max().item() <= 1e-12
    assert (torch.rsqrt(r.reshape(M, NCOL).square().mean(1) + EPS) - ref["rstd"]).abs().max().item() <= 1e-12


@pytest.mark.parametrize("M,K,with_dres", [(1, 64, True), (12, 128, False), (200, 384, True)])
def test_closed_form_backward_equals_autograd(M, K, with_dres):
    """Autograd of y = RMSNorm(residual + s * x) at x = anything (the adjoint does not depend on x beyond r), cotangents
    dy = P64 for y and dres_out for r: d residual = dres_in, d x = dx, d w = sum over rows of dy * xhat."""
    t = _data(M, K, "plain", seed=1)
    P, eps_x = R.product(t["A"], t["W"])
    g = torch.Generator().manual_seed(3)
    x = torch.randn(M, NCOL, generator=g, dtype=F64).requires_grad_()
    res = torch.randn(M, NCOL, generator=g, dtype=F64).requires_grad_()
    w = t["w"].double().requires_grad_()
    r = res + t["srow"][:, None] * x
    r.retain_grad()
    rstd = torch.rsqrt(r.square().mean(1) + EPS)
    y = r * rstd[:, None] * w
    loss = (y * P).sum()
    if with_dres:
        loss = loss + (r * t["dres_out"].double()).sum()
    loss.backward()
    b = R.backward_ref(P, eps_x, r.detach(), rstd.detach(), t["w"], t["dres_out"] if with_dres else None, t["srow"])
    assert (b["dres"] - res.grad).abs().max().item() <= 1e-12
    assert (b["dx"] - x.grad).abs().max().item() <= 1e-12
    assert (b["t"].sum(0) - w.grad).abs().max().item() <= 1e-12 * max(1.0, M ** 0.5)
    parts = torch.stack([b["t"][i].sum(0) for i in t["pw_rows"]])
    assert (parts.sum(0) - w.grad).abs().max().item() <= 1e-12 * max(1.0, M ** 0.5)


def test_pw_rows_partition_the_rows():
    for M in (1, 63, 64, 65, 100, 200, 513, 1472):
        nb = -(-M // R.TILE)
        rows = R.gemm_pw_rows(M, nb)
        assert sorted(torch.cat(rows).tolist()) == list(range(M))
        assert sorted(R.xcd_tile_of_block(b, nb) for b in range(nb)) == list(range(nb))
        assert max(len(i) for i in rows) <= R.TILE
    for B, rows_, cols, tr in ((1, 1, 1, False), (3, 5, 9, False), (2, 7, 9, True), (2, 14, 14, True), (1, 16, 16, False)):
        tiles = R.pooling_tile_rows(B, rows_, cols, tr)
        assert len(tiles) == B * -(-rows_ // 4)
        assert sorted(torch.cat(tiles).tolist()) == list(range(B * rows_ * cols))


def test_pooling_tiles_follow_the_token_geometry():
    # transposed 2 x 3 grid: memory token of (i, j) is i + 2 j
    assert R.pooling_tile_rows(1, 2, 3, True)[0].tolist() == [0, 2, 4, 1, 3, 5]
    assert [t.tolist() for t in R.pooling_tile_rows(2, 5, 2, False)] == [list(range(0, 8)), [8, 9], list(range(10, 18)), [18, 19]]


# ------------------------------------------------------------------------------------------------ emulation and mutations
SWEEP = [(M, K, fam) for M in (1, 200) for K in (64, 128, 384, 768, 1536) for fam in ("plain", "offset", "scaled")]


def _forward(t, A=None, mutate=None):
    """Comparators of the forward launch on the emulation's outputs (``mutate`` edits them first)."""
    P, eps_x = R.product(t["A"], t["W"])
    out = list(R.emulate_forward(t["A"] if A is None else A, t["W"], t["res"], t["srow"], t["w"], EPS))
    if mutate:
        out = mutate(out)
    rep = R.Report()
    R.check_forward(rep, P, eps_x, t["res"], t["srow"], t["w"], EPS, *out)
    return rep


def _backward(t, A=None, dres_out="given", mutate=None):
    P, eps_x = R.product(t["A"], t["W"])
    out = list(R.emulate_backward(t["A"] if A is None else A, t["W"], t["r"], t["rstd"], t["w"],
                                  t["dres_out"] if dres_out == "given" else dres_out, t["srow"], t["pw_rows"]))
    if mutate:
        out = mutate(out)
    rep = R.Report()
    R.check_backward(rep, P, eps_x, t["r"], t["rstd"], t["w"], t["dres_out"], t["srow"], *out, t["pw_rows"])
    return rep


@pytest.mark.parametrize("M,K,family", SWEEP)
def test_fp32_emulation_is_inside_every_bound(M, K, family):
    t = _data(M, K, family)
    f, b = _forward(t), _backward(t)
    print("forward", {k: round(v, 3) for k, v in f.ratio.items()}, "backward", {k: round(v, 3) for k, v in b.ratio.items()})
    assert f, f.msgs
    assert b, b.msgs
    # second phase and the patch-embed epilogue on the same operands
    T = R.emulate_forward(t["A"], t["W"], t["res"], t["srow"], t["w"], EPS)[2]
    g = torch.Generator().manual_seed(K)
    W2 = (torch.randn(R.K2, 128, generator=g) * R.K2 ** -0.5).bfloat16()
    rep = R.Report()
    R.check_second(rep, T, W2, (T.float() @ W2.float()).bfloat16())
    table = torch.randn(7, NCOL, generator=g)
    P, eps_x = R.product(t["A"], t["W"])
    R.check_rowbias(rep, P, eps_x, table, (t["A"].float() @ t["W"].float()).bfloat16().float() + table[torch.arange(M) % 7])
    assert rep, rep.msgs


def _drop_last_k_tile(t):
    A = t["A"].clone()
    A[:, -64:] = 0
    return A


@pytest.mark.parametrize("K", [128, 384, 1536])
def test_dropped_last_k_tile_fails(K):
    t = _data(200, K, "plain")
    f, b = _forward(t, A=_drop_last_k_tile(t)), _backward(t, A=_drop_last_k_tile(t))
    assert any("res_out" in m for m in f.msgs), f.msgs
    assert any("dres_in" in m for m in b.msgs) and any("pw" in m for m in b.msgs), b.msgs
    assert f.ratio["res_out"] > 100 and b.ratio["dres_in"] > 100


@pytest.mark.parametrize("K", [64, 384, 1536])
def test_one_percent_product_error_fails(K):
    t = _data(200, K, "plain")

    def fwd(out):       # res_out = residual + s * 1.01 h
        r, rstd, y = out
        h = (r - t["res"]) * 1.01
        return [t["res"] + h, rstd, y]

    f = _forward(t, mutate=fwd)
    assert any("res_out" in m for m in f.msgs), f.msgs
    b = _backward(t, A=(t["A"].float() * 1.01).bfloat16())
    assert any("dres_in" in m for m in b.msgs), b.msgs


def test_one_row_shift_fails():
    t = _data(200, 384, "plain")
    f = _forward(t, mutate=lambda o: [o[0].roll(1, 0), o[1], o[2]])
    assert any("res_out" in m for m in f.msgs), f.msgs
    f = _forward(t, mutate=lambda o: [o[0], o[1], o[2].roll(1, 0)])
    assert any(m.startswith("y") for m in f.msgs) and not any("res_out" in m for m in f.msgs), f.msgs
    b = _backward(t, mutate=lambda o: [o[0], o[1].roll(1, 0), o[2]])
    assert any(m.startswith("dx") for m in b.msgs), b.msgs


def test_omitted_dres_out_fails():
    t = _data(200, 384, "plain")
    b = _backward(t, dres_out=None)
    assert any("dres_in" in m for m in b.msgs) and any(m.startswith("dx") for m in b.msgs), b.msgs


def test_dres_in_times_the_droppath_scale_fails():
    t = _data(200, 384, "plain")
    b = _backward(t, mutate=lambda o: [o[0] * t["srow"].float()[:, None], o[1], o[2]])
    assert any("dres_in" in m for m in b.msgs) and not any(m.startswith("dx") for m in b.msgs), b.msgs


def test_pw_row_with_one_row_missing_fails():
    """At 200 rows the missing row is 1 / 64 of its workgroup's sum (ratio about 8) and would be 1 / 200 of the total."""
    t = _data(200, 384, "plain")

    def drop(o):
        rows = [i.clone() for i in t["pw_rows"]]
        rows[2] = rows[2][:-1]
        return [o[0], o[1], R.emulate_backward(t["A"], t["W"], t["r"], t["rstd"], t["w"], t["dres_out"], t["srow"], rows)[2]]

    b = _backward(t, mutate=drop)
    assert [m for m in b.msgs if m.startswith("pw")] and len(b.msgs) == 1, b.msgs
    assert "row 2 " in b.msgs[0], b.msgs
    # a whole workgroup's row dropped: the row count is checked
    b = _backward(t, mutate=lambda o: [o[0], o[1], o[2][:-1]])
    assert any("rows for" in m for m in b.msgs), b.msgs


def test_second_phase_and_rowbias_comparators_can_fail():
    t = _data(100, 384, "plain")
    T = R.emulate_forward(t["A"], t["W"], t["res"], t["srow"], t["w"], EPS)[2]
    g = torch.Generator().manual_seed(0)
    W2 = (torch.randn(R.K2, 128, generator=g) * R.K2 ** -0.5).bfloat16()
    C2 = (T.float() @ W2.float()).bfloat16()
    bad = C2.clone()
    bad[:, -8:] = 0
    rep = R.Report()
    R.check_second(rep, T, W2, bad)
    assert rep.msgs and "col 12" in rep.msgs[0], rep.msgs            # columns 120 .. 127
    rep = R.Report()                                                  # truncation instead of rounding: up to a whole ulp
    R.check_second(rep, T, W2, ((T.float() @ W2.float()).view(torch.int32) & -65536).view(torch.float32).bfloat16())
    assert rep.msgs
    table = torch.randn(13, NCOL, generator=g)
    P, eps_x = R.product(t["A"], t["W"])
    h32 = t["A"].float() @ t["W"].float()
    rep = R.Report()                                                  # the table of the wrong token
    R.check_rowbias(rep, P, eps_x, table, h32.bfloat16().float() + table[(torch.arange(100) + 1) % 13])
    assert rep.msgs
    rep = R.Report()                                                  # no rounding to bf16 before the add
    R.check_rowbias(rep, P, eps_x, table, h32 + table[torch.arange(100) % 13])
    assert len(rep.msgs) == 1 and "is bf16" in rep.msgs[0], rep.msgs
