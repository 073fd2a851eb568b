"""The dense-prediction operators (csrc/chan_ln.hip through fastvim_amd/dense_ops.py) against an unrounded fp64
reference, row by row, with the comparators and the derived bounds of ``norm_checks.py`` and no other tolerance.

* Feature tap: rows are tokens; the (B, C, H, W) result is brought back to (B*H*W, C).
* LN2d: rows are the (n, h, w) positions; input, output and gradients are permuted to (N*H*W, C).
"""
import pytest
import torch

import norm_checks as nc
from conftest import load_golden
from dense_recipe import LN2D_SHAPES, ln2d_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
FAMILIES = ("plain", "offset", "scaled", "zero_rows")      # the families without a DropPath scale (the ops have none)


def _ctx(msgs, **kw):
    return " ".join(f"{k}={v}" for k, v in kw.items()) + ": " + "; ".join(msgs)


def _rows(t):
    """(N, C, H, W) -> (N*H*W, C)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _maps(rows, N, H, W):
    """(N*H*W, C) -> contiguous (N, C, H, W)."""
    return rows.reshape(N, H, W, rows.shape[1]).permute(0, 3, 1, 2).contiguous()


def _family(family, B, Ltok, C, dt):
    """One input family as rows on the GPU: x (M, C) in ``dt`` (the sum of the family's x and residual), w, b, eps and
    the cotangent as fp32 rows."""
    inp = nc.make_inputs(family, B, Ltok, C, False, xdt=F32, res_dt=F32, with_scale=False)
    x = (inp["x"] + inp["residual"]).to(dt).to(DEV)
    return x, inp["w"].to(DEV), inp["b"].to(DEV), inp["eps"], inp["dy"].to(DEV)


def _nonfinite(out):
    return [f"{k} has non-finite values" for k, v in out.items() if not torch.isfinite(v).all()]


# ------------------------------------------------------------------------------------------------------ feature tap
def run_tap(x_rows, w, b, eps, dy_rows, B, H, W):
    from fastvim_amd.dense_ops import tap_layer_norm_nchw, tap_ln_forward
    C = x_rows.shape[1]
    hidden = x_rows.reshape(B, H * W, C).clone().requires_grad_()
    wp, bp = w.clone().requires_grad_(), b.clone().requires_grad_()
    y = tap_layer_norm_nchw(hidden, wp, bp, H, W, eps)
    assert y.shape == (B, C, H, W) and y.dtype == F32 and y.is_contiguous()
    y.backward(_maps(dy_rows, B, H, W))
    y2, mean, rstd, _, _ = tap_ln_forward(hidden.detach(), w, b, H, W, eps)
    assert torch.equal(y2, y.detach())
    assert hidden.grad.dtype == x_rows.dtype and hidden.grad.shape == hidden.shape
    return {"y": _rows(y.detach()), "mean": mean, "rstd": rstd, "dx": hidden.grad.reshape(-1, C), "dw": wp.grad, "db": bp.grad}


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,H,W", [(2, 4, 6), (2, 5, 7), (1, 1, 1), (2, 32, 32)])
@pytest.mark.parametrize("C", [192, 384, 768])
def test_tap_vs_fp64(C, B, H, W, dt):
    fails = []
    for family in FAMILIES:
        x, w, b, eps, dy = _family(family, B, H * W, C, dt)
        ref = nc.reference(x, w, b, None, None, eps, False, dy, None)
        out = run_tap(x, w, b, eps, dy, B, H, W)
        msgs = nc.check_all(out, ref, b) + _nonfinite(out)
        if family == "zero_rows" and not torch.equal(out["y"][::7], b.expand(len(out["y"][::7]), C)):
            msgs.append("y of an all-zero row is not exactly the bias")
        if msgs:
            fails.append(_ctx(msgs, family=family, C=C, grid=(B, H, W), dt=dt))
    assert not fails, "\n".join(fails)


def test_tap_token_l_is_cell_l_div_w_l_mod_w():
    """The layout itself, exactly: with weight 1, bias 0 the cell (h, w) of every plane holds token h * W + w."""
    from fastvim_amd.dense_ops import tap_layer_norm_nchw
    B, H, W, C = 2, 5, 7, 192
    x, w, b, eps, _ = _family("plain", B, H * W, C, F32)
    y = tap_layer_norm_nchw(x.reshape(B, H * W, C), w, b, H, W, eps)
    want = torch.nn.functional.layer_norm(x.double(), (C,), w.double(), b.double(), eps).reshape(B, H, W, C)
    for (bi, h, ww) in ((0, 0, 0), (0, 0, 6), (0, 1, 0), (1, 4, 6), (1, 2, 3)):
        assert (y[bi, :, h, ww].double() - want[bi, h, ww]).abs().max().item() < 1e-4, (bi, h, ww)


# ------------------------------------------------------------------------------------------------------------- LN2d
def run_ln2d(x_rows, w, b, eps, dy_rows, N, H, W):
    from fastvim_amd.dense_ops import ln2d_fn, ln2d_forward
    x = _maps(x_rows, N, H, W).requires_grad_()
    wp, bp = w.clone().requires_grad_(), b.clone().requires_grad_()
    y = ln2d_fn(x, wp, bp, eps)
    assert y.shape == x.shape and y.dtype == x.dtype and y.is_contiguous()
    y.backward(_maps(dy_rows, N, H, W))
    y2, mean, rstd, _, _ = ln2d_forward(x.detach(), w, b, eps)
    assert torch.equal(y2, y.detach())
    assert x.grad.dtype == x.dtype
    return {"y": _rows(y.detach()), "mean": mean, "rstd": rstd, "dx": _rows(x.grad), "dw": wp.grad, "db": bp.grad}


def _ln2d_cases():
    for shape in LN2D_SHAPES:
        yield shape, F32
        if shape[1] in (96, 256, 384):
            yield shape, BF16


LN2D_CASES = list(_ln2d_cases())
LN2D_IDS = ["x".join(map(str, s)) + ("-bf16" if d == BF16 else "-fp32") for s, d in LN2D_CASES]


@pytest.mark.parametrize("shape,dt", LN2D_CASES, ids=LN2D_IDS)
def test_ln2d_vs_fp64(shape, dt):
    N, C, H, W = shape
    fails = []
    for family in FAMILIES:
        x, w, b, eps, dy = _family(family, N, H * W, C, dt)
        dy = dy.to(dt)                                   # the cotangent arrives in y's dtype
        ref = nc.reference(x, w, b, None, None, eps, False, dy, None)
        out = run_ln2d(x, w, b, eps, dy, N, H, W)
        msgs = nc.check_all(out, ref, b) + _nonfinite(out)
        if msgs:
            fails.append(_ctx(msgs, family=family, shape=shape, dt=dt))
    assert not fails, "\n".join(fails)


@pytest.fixture(scope="module")
def recorded():
    d = load_golden("dense.pt")["ln2d"]
    return d, load_golden(d["maps_file"])


@pytest.mark.parametrize("shape,dt", LN2D_CASES, ids=LN2D_IDS)
def test_ln2d_vs_recorded_reference(shape, dt, recorded):
    """The reference class's own fp64 output and gradients (tests/golden/gen_dense.py) under the same bounds; the two
    largest maps are recorded at 32 positions (all channels), input gradients of the larger maps at 8."""
    meta, maps = recorded
    N, C, H, W = shape
    rec, mp = meta["cases"][shape], maps[shape]
    x4, dy4, w, b = ln2d_inputs(shape, rec["seed"])
    x, dy = _rows(x4).to(dt).to(DEV), _rows(dy4).to(dt).to(DEV)
    w, b = w.to(DEV), b.to(DEV)
    ref = nc.reference(x, w, b, None, None, meta["eps"], False, dy, None)        # per-row cond and bound terms
    out = run_ln2d(x, w, b, meta["eps"], dy, N, H, W)

    def at(idx, **recorded_values):
        sel = (lambda t: t) if idx is None else (lambda t: t[idx.to(DEV)])
        sub = dict(ref, cond=sel(ref["cond"]))
        sub.update({k: v.to(DEV) for k, v in recorded_values.items()})
        return sub, sel

    sub, sel = at(rec["rows"], y=mp["y_rows"])
    msgs = [nc.check_y(sel(out["y"]), sub, b)]
    sub, sel = at(rec["dx_rows"], dx=mp["dx_rows"])
    msgs.append(nc.check_dx(sel(out["dx"]), sub))
    msgs.append(nc.check_dw(out["dw"], dict(ref, dw=rec["dw"].to(DEV))))
    msgs.append(nc.check_db(out["db"], dict(ref, db=rec["db"].to(DEV))))
    msgs = [m for m in msgs if m]
    assert not msgs, _ctx(msgs, shape=shape, dt=dt)


# ------------------------------------------------------------------------------------------------------ determinism
def test_two_runs_are_bit_identical():
    x, w, b, eps, dy = _family("plain", 2, 35, 384, BF16)
    a, c = run_tap(x, w, b, eps, dy, 2, 5, 7), run_tap(x, w, b, eps, dy, 2, 5, 7)
    for k in a:
        assert torch.equal(a[k], c[k]), f"tap {k} differs between two runs"
    x, w, b, eps, dy = _family("plain", 3, 49, 256, F32)
    a, c = run_ln2d(x, w, b, eps, dy, 3, 7, 7), run_ln2d(x, w, b, eps, dy, 3, 7, 7)
    for k in a:
        assert torch.equal(a[k], c[k]), f"LN2d {k} differs between two runs"


# ------------------------------------------------------------------------------------- direct weight-gradient route
def test_tap_weight_gradient_goes_into_the_flat_state():
    """Under a FlatTrainingState ``outnorm_0.weight`` carries ``_fv_direct`` and a view of the flat gradient: the tap's
    backward reduces its partial rows into that view (on top of what is there) and hands autograd no dw."""
    from fastvim_amd.fastvim import MM_FastVim
    from fastvim_amd.flat import FlatTrainingState
    from fastvim_amd.mixer_ops import pending_reductions
    torch.manual_seed(5)
    C, H, W = 192, 4, 6
    m = MM_FastVim(img_size=(64, 96), depth=2, embed_dim=C, out_indices=[1], fused_add_norm=True, residual_in_fp32=True,
                   drop_path_rate=0.0).to(DEV).train()
    with torch.no_grad():
        m.outnorm_0.weight.copy_(1 + 0.1 * torch.randn(C))
        m.outnorm_0.bias.copy_(0.1 * torch.randn(C))
    x = torch.randn(2, 3, 64, 96, device=DEV)
    g = torch.randn(2, C, H, W, device=DEV)
    preset = torch.randn(C, generator=torch.Generator().manual_seed(7)).to(DEV)
    with FlatTrainingState(m) as flat:
        wgt = m.outnorm_0.weight
        assert getattr(wgt, "_fv_direct", False) and wgt.grad is not None
        with torch.no_grad():
            hidden = m.forward_features(x, out_indices=m.out_indices)[0][0]
        flat.zero_grad()
        wgt.grad.copy_(preset)
        storage = wgt.grad.data_ptr()
        out = m(x)
        assert torch.is_tensor(out) and out.shape == (2, C, H, W)
        out.backward(g)
        flat.finish_backward()
        assert pending_reductions() == 0, "gradient reductions are still queued after finish_backward()"
        assert wgt.grad.data_ptr() == storage, ".grad was replaced, not accumulated into"
        got = wgt.grad.detach().clone()
        w, b = wgt.detach().clone(), m.outnorm_0.bias.detach().clone()
    ref = nc.reference(hidden.reshape(-1, C), w, b, None, None, m.outnorm_0.eps, False, _rows(g), None)
    want = ref["dw"] + preset.double()
    msg = nc.check_dw(got, dict(ref, dw=want), extra=2.0 ** -24 * want.abs())     # one fp32 rounding of preset + dw
    assert not msg, msg


# ------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors():
    from fastvim_amd.dense_ops import ln2d_fn, tap_layer_norm_nchw
    one = lambda n: torch.ones(n, device=DEV)
    with pytest.raises(RuntimeError, match="C = 0"):
        ln2d_fn(torch.zeros(2, 0, 3, 3, device=DEV), one(0), one(0))
    with pytest.raises(RuntimeError, match="C = 1025"):
        ln2d_fn(torch.zeros(2, 1025, 2, 2, device=DEV), one(1025), one(1025))
    with pytest.raises(RuntimeError, match="C = 0"):
        tap_layer_norm_nchw(torch.zeros(2, 6, 0, device=DEV), one(0), one(0), 2, 3)
    with pytest.raises(RuntimeError, match="C = 190"):
        tap_layer_norm_nchw(torch.zeros(2, 6, 190, device=DEV), one(190), one(190), 2, 3)
    with pytest.raises(RuntimeError, match="is not"):
        tap_layer_norm_nchw(torch.zeros(2, 7, 192, device=DEV), one(192), one(192), 2, 3)
    with pytest.raises(RuntimeError, match="elements"):
        ln2d_fn(torch.zeros(2, 96, 2, 2, device=DEV), one(95), one(96))
    with pytest.raises(RuntimeError, match="fp32 or bf16"):
        ln2d_fn(torch.zeros(2, 96, 2, 2, device=DEV, dtype=torch.float16), one(96), one(96))
    with pytest.raises(RuntimeError, match="GPU only"):
        ln2d_fn(torch.zeros(2, 96, 2, 2), one(96), one(96))
    with pytest.raises(RuntimeError, match="GPU only"):
        tap_layer_norm_nchw(torch.zeros(2, 6, 192), one(192), one(192), 2, 3)


def test_noncontiguous_inputs_are_read_by_their_strides():
    """A strided view is made contiguous before the launch: same bits as the contiguous copy, forward and backward."""
    from fastvim_amd.dense_ops import ln2d_fn, tap_layer_norm_nchw
    x, w, b, eps, dy = _family("plain", 2, 35, 192, F32)
    wide = torch.randn(2, 35, 2 * 192, device=DEV)
    wide[..., ::2] = x.reshape(2, 35, 192)
    view = wide[..., ::2].requires_grad_()
    assert not view.is_contiguous()
    dense = x.reshape(2, 35, 192).clone().requires_grad_()
    ya, yb = tap_layer_norm_nchw(view, w, b, 5, 7, eps), tap_layer_norm_nchw(dense, w, b, 5, 7, eps)
    assert torch.equal(ya, yb)
    gmap = _maps(dy, 2, 5, 7)
    ya.backward(gmap.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2))     # a non-contiguous cotangent too
    yb.backward(gmap)
    assert torch.equal(view.grad, dense.grad)
    xm = _maps(x, 2, 5, 7)
    cl = xm.to(memory_format=torch.channels_last).requires_grad_()
    assert not cl.is_contiguous()
    xm.requires_grad_()
    ya, yb = ln2d_fn(cl, w, b, eps), ln2d_fn(xm, w, b, eps)
    assert torch.equal(ya, yb)
    ya.backward(gmap.to(memory_format=torch.channels_last))
    yb.backward(gmap)
    assert torch.equal(cl.grad, xm.grad)
