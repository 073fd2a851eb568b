"""Pins the float64 family references of ``mixer_family_ref.py`` to ``oracle.fastvim_mixer_oracle`` and the case table
of ``test_mixer_families_gpu.py`` to the dispatcher (``fv_mixer_plan``, host code only).  No GPU.

The pin composes the four reference functions -- conv + pool, combine and their two adjoints -- with the x_proj / dt_proj /
selective-scan glue of ``oracle/mixer.py`` into a whole mixer, forward AND backward (the backward is the chain of the
two adjoint functions, not autograd through the forward ones), and asserts that output, d hidden and every parameter
gradient equal those of ``fastvim_mixer_oracle`` to 1e-12: a reference that is itself wrong cannot agree with a wrong
kernel."""
import pytest
import torch
import torch.nn.functional as F

import mixer_family_ref as R
import test_mixer_families_gpu as G
from oracle import fastvim_mixer_oracle
from oracle.scan import selective_scan_oracle

F64 = torch.float64


def _params(d_model, N, gen):
    d_in, Rk = 2 * d_model, max(1, d_model // 16)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=F64)
    p = {"in_proj.weight": rn(2 * d_in, d_model) / d_model ** 0.5, "out_proj.weight": rn(d_model, d_in) / d_in ** 0.5,
         "layernorm.weight": 1 + 0.1 * rn(d_in), "layernorm.bias": 0.1 * rn(d_in)}
    for s in ("", "_b"):
        p[f"conv1d{s}.weight"] = 0.5 * rn(d_in, 1, 4)
        p[f"conv1d{s}.bias"] = 0.2 * rn(d_in)
        p[f"x_proj{s}.weight"] = rn(Rk + 2 * N, d_in) / d_in ** 0.5
        p[f"dt_proj{s}.weight"] = rn(d_in, Rk)
        p[f"dt_proj{s}.bias"] = 0.3 * rn(d_in) - 2.0
        p[f"A{s}_log"] = torch.log(torch.arange(1, N + 1, dtype=F64)).repeat(d_in, 1) + 0.1 * rn(d_in, N)
        p[f"D{s}"] = 1 + 0.1 * rn(d_in)
    return p


class _StaysF64(torch.Tensor):
    """The oracle takes A_log, D and dt_proj.bias through ``.float()`` (their storage type in the models), which would
    round their values and, on the way back, their gradients to fp32.  The pin is a float64 statement: these parameters
    reach the oracle as a Tensor subclass whose ``.float()`` is the identity."""

    def float(self):
        return self


def _scan_glue(xc, p):
    """yc (2, B, Lc, d_in) from xc (2, B, Lc, d_in): x_proj -> dt_proj -> selective scan per direction, the backward
    direction over the pooled positions in descending order (oracle/mixer.py:74-93)."""
    ys = []
    for k, sfx in enumerate(("", "_b")):
        pooled = xc[k].permute(0, 2, 1)                                    # (B, d_in, Lc)
        Bsz, d_in, Lc = pooled.shape
        Wx, Wdt = p[f"x_proj{sfx}.weight"], p[f"dt_proj{sfx}.weight"]
        Rk = Wdt.shape[1]
        N = (Wx.shape[0] - Rk) // 2
        x_dbl = pooled.permute(0, 2, 1).reshape(Bsz * Lc, d_in) @ Wx.t()
        dt = (x_dbl[:, :Rk] @ Wdt.t()).reshape(Bsz, Lc, d_in).permute(0, 2, 1)
        Bm = x_dbl[:, Rk:Rk + N].reshape(Bsz, Lc, N).permute(0, 2, 1)
        Cm = x_dbl[:, Rk + N:].reshape(Bsz, Lc, N).permute(0, 2, 1)
        A = -torch.exp(p[f"A{sfx}_log"])
        y = selective_scan_oracle(pooled, dt, A, Bm, Cm, None, None, p[f"dt_proj{sfx}.bias"], True, False,
                                  compute_dtype=F64, out_dtype=F64, reverse=bool(k))
        ys.append(y.permute(0, 2, 1))
    return torch.stack(ys)


PIN = {
    "3x5": dict(grid=(3, 5)),
    "3x5_transposed": dict(grid=(3, 5), transposed=True),
    "2x4_tpp2": dict(grid=(2, 4), tpp=2),
    "2x4_tpp2_transposed": dict(grid=(2, 4), tpp=2, transposed=True),
    "3x5_max": dict(grid=(3, 5), collapse="max"),
    "2x4_tpp2_max_transposed": dict(grid=(2, 4), tpp=2, collapse="max", transposed=True),
    "3x5_no_norm": dict(grid=(3, 5), norm=False),
    "3x5_scaling": dict(grid=(3, 5), scaling=0.375),
    "2x4_tpp2_no_norm_scaling": dict(grid=(2, 4), tpp=2, norm=False, scaling=2.5),
}


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


@pytest.mark.parametrize("name", list(PIN))
def test_composed_family_references_reproduce_the_mixer_oracle(name):
    cfg = PIN[name]
    rows, cols = cfg["grid"]
    tpp, transposed = cfg.get("tpp", 1), cfg.get("transposed", False)
    pool_max, norm, scaling = cfg.get("collapse", "mean") == "max", cfg.get("norm", True), cfg.get("scaling", 1)
    d_model, N, Bsz = 16, 4, 2
    d_in, Ltok = 2 * d_model, rows * cols * tpp
    gen = torch.Generator().manual_seed(len(name))
    p0 = _params(d_model, N, gen)
    h = torch.randn(Bsz, Ltok, d_model, generator=gen, dtype=F64)
    gy = torch.randn(Bsz, Ltok, d_model, generator=gen, dtype=F64)

    # the oracle, sequence order
    p = {k: v.clone().requires_grad_() for k, v in p0.items()}
    hs = h.clone().requires_grad_()
    y_ref = fastvim_mixer_oracle({k: v.as_subclass(_StaysF64) for k, v in p.items()}, hs, (rows, cols), tokens_per_patch=tpp, collapse_method="max" if pool_max else "mean",
                                 scaling_factor=scaling, use_norm_after_ssm=norm, compute_dtype=F64, out_dtype=F64)
    y_ref.backward(gy)

    # memory order: the transposed grid is the oracle's sequence with its cells permuted (tests/test_mixer_gpu.py)
    if transposed:
        perm = lambda t: t.reshape(Bsz, rows, cols, tpp, -1).transpose(1, 2).reshape(Bsz, Ltok, -1)
    else:
        perm = lambda t: t
    hm, gym = perm(h), perm(gy)
    q = {k: v.clone() for k, v in p0.items()}
    cw, cwb = q["conv1d.weight"].reshape(d_in, 4), q["conv1d_b.weight"].reshape(d_in, 4)
    lw, lb = (q["layernorm.weight"], q["layernorm.bias"]) if norm else (None, None)
    geo = dict(rows=rows, cols=cols, tpp=tpp, transposed=transposed)

    # forward: the two forward references around the scan glue
    xz = hm @ q["in_proj.weight"].t()
    x, z = xz[..., :d_in], xz[..., d_in:]
    _, _, xc, skip, arg = R.conv_pool_ref(x, cw, q["conv1d.bias"], cwb, q["conv1d_b.bias"], q["D"], q["D_b"],
                                          pool_max=pool_max, scaling=scaling, **geo)
    glue = {k: v.clone().requires_grad_() for k, v in q.items() if k.startswith(("x_proj", "dt_proj", "A_"))}
    xc_leaf = xc.clone().requires_grad_()
    yc = _scan_glue(xc_leaf, glue)
    o, g, mean, rstd = R.combine_ref(z, skip, yc.detach(), lw, lb, 1e-5, **geo)
    y = g @ q["out_proj.weight"].t()
    assert _rel(y, perm(y_ref.detach())) <= 1e-12
    if norm:      # the saved statistics are those of the normalisation the output went through
        assert _rel(((o - mean.view(Bsz, Ltok, 1)) * rstd.view(Bsz, Ltok, 1) * lw + lb) * F.silu(z), g) <= 1e-12

    # backward: the two adjoint references around autograd through the glue
    dg = gym @ q["out_proj.weight"]
    dz, d_o, dyc, dlw, dlb = R.combine_adjoint_ref(dg, z, skip, yc.detach(), lw, lb, 1e-5, **geo)
    yc.backward(torch.stack([dyc, dyc]))
    dx, part = R.conv_pool_adjoint_ref(x, cw, q["conv1d.bias"], cwb, q["conv1d_b.bias"], q["D"], q["D_b"], d_o, xc_leaf.grad,
                                       pool_max=pool_max, scaling=scaling, amax=arg, **geo)
    dxz = torch.cat([dx, dz], -1)
    got = {"in_proj.weight": dxz.reshape(-1, 2 * d_in).t() @ hm.reshape(-1, d_model),
           "out_proj.weight": gym.reshape(-1, d_model).t() @ g.reshape(-1, d_in),
           "conv1d.weight": part[:4 * d_in].view(d_in, 1, 4), "conv1d_b.weight": part[4 * d_in:8 * d_in].view(d_in, 1, 4),
           "conv1d.bias": part[8 * d_in:9 * d_in], "conv1d_b.bias": part[9 * d_in:10 * d_in],
           "D": part[10 * d_in:11 * d_in], "D_b": part[11 * d_in:]}
    if norm:
        got["layernorm.weight"], got["layernorm.bias"] = dlw, dlb
    got.update({k: v.grad for k, v in glue.items()})
    assert _rel(dxz @ q["in_proj.weight"], perm(hs.grad)) <= 1e-12
    for k, v in p.items():
        if v.grad is None:
            assert not norm and k.startswith("layernorm"), k
            continue
        assert _rel(got[k], v.grad) <= 1e-12, (k, _rel(got[k], v.grad))
    assert set(got) == {k for k, v in p.items() if v.grad is not None}


def test_dxc2_is_a_second_addend_of_the_pooled_gradient():
    gen = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=F64)
    d, rows, cols = 8, 2, 14
    args = (rn(2, rows * cols, d), rn(d, 4), rn(d), rn(d, 4), rn(d), rn(d), rn(d), rn(2, rows * cols, d))
    a, b = rn(2, 2, rows, d), rn(2, 2, rows, d)
    dx1, p1 = R.conv_pool_adjoint_ref(*args, a, rows, cols, dxc2=b)
    dx2, p2 = R.conv_pool_adjoint_ref(*args, a + b, rows, cols)
    dx3, _ = R.conv_pool_adjoint_ref(*args, a, rows, cols)
    assert _rel(dx1, dx2) <= 1e-14 and _rel(p1, p2) <= 1e-14 and _rel(dx3, dx2) > 1e-2


# ------------------------------------------------------------------------------------------------ the case table
@pytest.fixture(scope="module")
def lib():
    import fastvim_amd.build as fb
    fb.build()
    from fastvim_amd import _lib
    return _lib.lib()


def test_case_table_states_the_dispatchers_plans(lib):
    """What the GPU tests assert before they launch, checked here without a GPU; a family a case leaves out has no
    plan at that shape -- or the case is one of the forward-only rows shorter than the conv halo."""
    for c in G.CASES:
        for fam in range(4):
            if fam in c["plans"]:
                G.assert_plan(lib, c, fam)
            elif "short" in c["opts"]:
                assert fam in (G.COMB_BWD, G.CONV_BWD) and c["cols"] * c["tpp"] < 3, c["name"]
            else:
                assert G.query_plan(lib, fam, c["B"], c["rows"], c["cols"], c["tpp"], c["d"], c["pm"], c["dt"])[0] == 0, (c["name"], fam)
        if G.CONV_BWD in c["plans"]:
            assert c["cols"] * c["tpp"] >= 3, c["name"]
        if G.COMB_BWD in c["plans"]:
            assert G.COMB_FWD in c["plans"], c["name"]
        if G.COMB_FWD in c["plans"]:
            assert G.CONV_FWD in c["plans"], c["name"]


SWEEP_D = (40, 64, 96, 128, 192, 256, 320, 384, 512, 640, 768, 1024, 1088, 1280, 1536, 2048, 2560, 3072)
SWEEP_COLS = (1, 2, 3, 5, 14, 16, 24, 32)
SWEEP_TPP = (1, 2, 8)


def test_every_plan_key_of_the_sweep_has_a_case(lib):
    """Path completeness by the dispatcher's own description: every distinct supported key
    (family, form, vec, slabs > 1, tpp > 1, pool_max, dtype where the plan depends on it) of the sweep occurs in the
    case table.  (The adjoint launchers refuse fewer than 3 tokens per pooling row whatever the plan says: no key
    is reachable only through such a shape.)"""
    keys = {}
    for fam in range(4):
        for d in SWEEP_D:
            for cols in SWEEP_COLS:
                for tpp in SWEEP_TPP:
                    for pm in (0, 1):
                        for dt in ("f32", "bf16"):
                            k = G.plan_key(lib, fam, 3, cols, tpp, d, pm, dt)
                            if k is not None:
                                keys.setdefault(k, (d, cols, tpp, pm, dt))
    covered = {}
    for c in G.CASES:
        for fam in c["plans"]:
            covered.setdefault(G.stated_key(lib, c, fam), c["name"])
    missing = {k: v for k, v in keys.items() if k not in covered}
    assert not missing, f"{len(missing)} of {len(keys)} plan keys without a case (key: first shape d, cols, tpp, max, dtype): {missing}"
    for k in sorted(keys, key=str):
        print(k, "<-", covered[k])


def test_max_pool_seeds_have_few_near_ties():
    """The near-tie excuse of the argmax comparison (float64 top two closer than 1e-5 * max(1, |top|)) covers at most
    0.5 % of the pooling groups of every max-pooling case, on the reference alone: seeds 1000 + position in CASES."""
    for c in G.CASES:
        if not c["pm"]:
            continue
        inp = G.make_inputs(c)
        conv_f, conv_b, *_ = R.conv_pool_ref(inp["xz"][..., :c["d"]], inp["cw"], inp["cb"], inp["cwb"], inp["cbb"], None, None,
                                             c["rows"], c["cols"], c["tpp"], True, 1.0, c["tr"])
        tie = torch.stack([G.near_tie_groups(conv_f, c), G.near_tie_groups(conv_b, c)])
        assert tie.float().mean().item() <= 0.005, (c["name"], tie.float().mean().item())


def test_offset_cases_carry_thirty_standard_deviations():
    for c in G.CASES:
        if "offset" not in c["opts"]:
            continue
        inp = G.make_inputs(c)
        skip = R.conv_pool_ref(inp["xz"][..., :c["d"]], inp["cw"], inp["cb"], inp["cwb"], inp["cbb"], inp["D"], inp["Db"],
                               c["rows"], c["cols"], c["tpp"], c["pm"], inp["scaling"], c["tr"])[3]
        o = R.combine_ref(inp["xz"][..., c["d"]:], skip.to(G.DT[c["dt"]]), inp["yc"], None, None, 1e-5, c["rows"], c["cols"],
                          c["tpp"], c["tr"])[0]
        assert (o.mean(-1).abs() / o.std(-1)).min().item() >= 30.0, c["name"]
    forms = {c["plans"][G.COMB_FWD][:2] for c in G.CASES if "offset" in c["opts"]}
    assert {f[0] for f in forms} >= {G.FORMS["G"], G.FORMS["W"]}
