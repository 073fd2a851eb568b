"""CPU side of test_scan_cl_plans_gpu.py: the float64 reference of ``scan_cl_ref.py`` pinned to
``oracle.selective_scan_oracle``; the case table against the dispatcher (every case has the keys it states, every key
the queries reach has a case, the edges are there); a plain fp32 emulation of the same recurrence inside every bound on
every GPU case's inputs (bounds that fp32 arithmetic itself could not keep would say nothing about a kernel); and
mutations of reference outputs that each comparison must notice."""
import itertools

import pytest
import torch

import scan_cl_ref as S
import test_scan_cl_plans_gpu as G
from oracle.scan import selective_scan_oracle

N, F64 = S.N, torch.float64


# ------------------------------------------------------------------------------------------------ reference == oracle
def _oracle(inp, k, dyc=None, steps=None):
    """Direction k through selective_scan_oracle (its own walk: ``reverse``), fp64 autograd.  ``steps``: only the first
    ``steps`` steps of the walk (the prefix whose last state a checkpoint holds) -> the last state."""
    B, Lc, d, R = inp["B"], inp["Lc"], inp["d_in"], inp["R"]
    rows = slice(None) if steps is None else (slice(Lc - steps, Lc) if k else slice(0, steps))
    u = inp["xc"][k].double()[:, rows].clone().requires_grad_()
    xd = inp["x_dbl"][k].view(B, Lc, -1).double()[:, rows].clone().requires_grad_()
    W_, b_, Al = (inp[n][k].double().clone().requires_grad_() for n in ("Wdt", "bdt", "A_log"))
    delta = xd[..., :R] @ W_.t()
    y, last = selective_scan_oracle(u.transpose(1, 2), delta.transpose(1, 2), -torch.exp(Al), xd[..., R:R + N].transpose(1, 2),
                                    xd[..., R + N:].transpose(1, 2), None, None, b_, True, return_last_state=True,
                                    compute_dtype=F64, out_dtype=F64, reverse=bool(k))
    if steps is not None:
        return last
    g = inp["dyc"].expand(2, B, Lc, d)[k] if dyc is None else dyc[k]
    y.transpose(1, 2).backward(g.double())
    return y.transpose(1, 2).detach(), u.grad, xd.grad.reshape(B * Lc, -1), Al.grad, W_.grad, b_.grad


def _close12(a, b):
    assert (a - b).abs().max().item() <= 1e-12 * max(1.0, b.abs().max().item()), (a - b).abs().max().item()


SHAPES = [(2, 5, 24, 3, False), (3, 17, 40, 7, True), (2, 37, 72, 13, False), (1, 14, 64, 49, False), (4, 1, 200, 1, False)]


@pytest.mark.parametrize("B,Lc,d,R,dpd", SHAPES)
def test_reference_equals_the_selective_scan_oracle(B, Lc, d, R, dpd):
    inp = S.make_inputs(B, Lc, d, R, False, seed=B + Lc, dyc_per_direction=dpd)
    ref = S.reference(inp, per_element=False)
    for k in range(2):
        y, du, dxd, dA, dW, db = _oracle(inp, k)
        for a, b in ((ref["y"][k], y), (ref["du"][k], du), (ref["dx_dbl"][k], dxd)):
            _close12(a, b)
        _close12(ref["rows"].view(2, -1)[k], torch.cat([dA.reshape(-1), dW.reshape(-1), db.reshape(-1)]))
        # checkpoints: the state entering chunk c is the oracle's last state on the first 16 c steps of the walk
        assert ref["ckpt"].shape[2] == -(-Lc // 16) and not ref["ckpt"][:, :, 0].any()
        for c in range(1, ref["ckpt"].shape[2]):
            _close12(ref["ckpt"][k, :, c], _oracle(inp, k, steps=16 * c))
        # ... and the state after EVERY step, in walk order
        for s in (0, Lc // 2, Lc - 1):
            _close12(ref["states"][k, :, s], _oracle(inp, k, steps=s + 1))


@pytest.mark.parametrize("B,Lc,d,R,dpd", SHAPES[:3])
def test_masked_pieces_are_the_masked_gradients_and_sum_to_the_whole(B, Lc, d, R, dpd):
    inp = S.make_inputs(B, Lc, d, R, False, seed=7 + d, dyc_per_direction=dpd)
    ref = S.reference(inp, chunk_channels=16)
    whole = S.reference(inp, per_element=False)
    assert ref["slices"].shape[0] == -(-d // 16)
    _close12(ref["slices"].sum(0), ref["dx_dbl"])
    _close12(ref["rows"].sum(0, keepdim=True), whole["rows"])
    _close12(ref["dx_dbl"], whole["dx_dbl"])
    g = inp["dyc"].expand(2, B, Lc, d)
    for b in range(B):      # the parameter copy of element b receives the gradient of dyc masked to element b
        m = torch.zeros(B, 1, 1)
        m[b] = 1
        _close12(S.reference(inp, per_element=False, dyc=g * m)["rows"][0], ref["rows"][b])
    m = torch.zeros(d)
    m[16:32] = 1            # a slice is the gradient of dyc masked to its channels, against the oracle as well
    for k in range(2):
        _close12(ref["slices"][1][k], _oracle(inp, k, dyc=g * m)[2])
    _close12(S.group_rows(ref["rows"], 1), ref["rows"])
    if B % 2 == 0:
        _close12(S.group_rows(ref["rows"], 2)[0], ref["rows"][0] + ref["rows"][1])


# ------------------------------------------------------------------------------------------------ the case table and the dispatcher
@pytest.fixture(scope="module")
def q():
    import fastvim_amd.build as fb
    fb.build()
    from fastvim_amd import _lib
    return G.Queries(_lib.lib())


def test_case_table_states_the_dispatchers_keys(q):
    for c in G.CASES:
        G.assert_keys(q, c)


GRID = dict(B=(1, 2, 3, 4, 64, 128, 132, 256, 260, 512, 516),
            Lc=(1, 2, 13, 14, 15, 16, 17, 32, 33, 37, 128, 129, 240, 241, 400),
            d=(24, 32, 40, 64, 72, 192, 200, 224, 384, 416, 576, 768, 800, 1536),
            R=(1, 2, 7, 12, 13, 24, 25, 48, 49, 80, 96))


def test_every_key_the_queries_reach_has_a_case(q):
    """The product's dispatch over a grid that holds every boundary of the rules (rank classes 12 | 13, 24 | 25, 48 | 49;
    Lc 13 .. 17; the NBB batches; 192-channel multiples; the fused launch's d_inner % 32 and <= 768; the segment
    threshold 240 | 241): the fused forward wherever its query says yes, the fold wherever its query says yes (and the
    unfolded short kernel there too), checkpoints wanted / given or not, the workspace as the product passes it."""
    have_f = {k for c in G.CASES for k in c["fwd"]}
    have_b = {k for c in G.CASES for k in c["bwd"]}
    reach_f, reach_b = set(), set()
    for B, Lc, d, R in itertools.product(*GRID.values()):
        for dt in G.DTS:
            for flag in (False, True):
                reach_f.add(q.fwd_key(B, Lc, d, R, dt, want_ckpt=flag))
                reach_b.add(q.bwd_key(B, Lc, d, R, dt, given=flag))
            if q.fold_ok(B, Lc, d, R, dt):
                reach_b.add(q.bwd_key(B, Lc, d, R, dt, fold=True))
    assert G.LEFT_OUT <= reach_b and not (G.LEFT_OUT & have_b)
    assert reach_f == have_f, (sorted(reach_f - have_f, key=str), sorted(have_f - reach_f, key=str))
    assert reach_b - G.LEFT_OUT == have_b, (sorted(reach_b - G.LEFT_OUT - have_b, key=str), sorted(have_b - reach_b, key=str))
    assert len(have_f) == 36 + 24 + 8 and len(have_b) == 96 + 8 + 24 + 6 + 4
    # the generic backward below dt_rank 49 is reached through the tuning variables only: no such key here
    assert not any(k[0] == "generic" and k[2] != 24 for k in reach_b)


def test_the_edges_are_in_the_table():
    by = lambda *kinds: [c for c in G.CASES if c["kind"] in kinds]
    assert {c["Lc"] for c in by("short")} >= {1, 2, 13, 14, 15, 16}
    assert {c["Lc"] for c in by("chunked")} >= {17, 32, 33, 37} and {c["Lc"] for c in by("seg")} == {241, 400}
    assert {c["R"] for c in G.CASES} >= {1, 2, 7, 12, 13, 24, 25, 48, 49, 80, 96}
    # each kind on its own: lanes and waves past the row, and rows wider than one workgroup with a tail chunk of 8
    assert {c["d"] for c in by("short")} >= {24, 40, 72, 200, 392} and {c["d"] for c in by("chunked")} >= {40, 72, 200}
    assert any(c["d"] % 16 for c in by("generic")) and any(c["d"] % 16 for c in by("seg"))
    for dt in G.DTS:
        for rc in (3, 6, 12):
            for lcc, exact in ((14, True), (14, False), (16, True), (16, False)):
                # the 192-channel short backward on two or three workgroups, the last one 8 channels wide
                assert any(c["d"] > 192 and c["d"] % 192 == 8 and c["bwd"][0][1:5] == (dt, rc, lcc, exact) for c in by("short"))
            # ... and the generic forward that rides on the short shapes on more than one 64-channel block, ragged last one
            assert any(c["d"] > 64 and c["d"] % 64 and c["fwd"] == (("generic", dt, rc),) for c in by("short"))
    assert {c["Lc"] for c in by("chunked") if c["bwd"][0][3] == 4} >= {17, 32, 33, 37}
    assert all(any(c["d"] > 192 and c["nbb"] == n for c in by("short")) for n in (1, 2, 4, 8))
    assert {c["R"] for c in by("short") if c["nbb"] <= 2} >= {1, 2, 7, 12, 13, 24, 25, 48}
    assert any(c["B"] > 1 for c in by("seg"))      # (element, segment) row order is told from (segment, element)
    assert {c["d"] for c in by("fused")} == {32, 64, 224, 384, 416, 576, 768} and {c["Lc"] for c in by("fused")} == {1, 9, 14, 15, 16}
    assert {c["R"] for c in by("fused")} == {1, 2, 7, 12, 13, 24, 25, 48}
    assert {(c["B"], c["Lc"], c["d"], c["R"]) for c in G.CASES} >= {
        (128, 14, 64, 48), (132, 14, 64, 48), (128, 17, 64, 2), (128, 33, 200, 6), (1, 241, 64, 2), (1, 400, 72, 6), (2, 14, 72, 64),
        (2, 14, 64, 80), (2, 24, 64, 49), (2, 25, 64, 49), (1, 128, 64, 96)}
    assert all(c["Lc"] <= 400 for c in G.CASES)
    kinds_dpd = {c["bwd"][0][0] + (c["bwd"][0][-1] if c["kind"] == "generic" else "") for c in G.CASES if c["dpd"]}
    assert kinds_dpd == {"short", "chunked", "chunked_seg", "genericlds", "genericglobal"}


# ------------------------------------------------------------------------------------------------ fp32 emulation inside the bounds
def _emulate(c, rep):
    inp = G.make_inputs(c)
    if c["kind"] == "fused":
        P, bound = S.fused_xdbl_ref(inp["xc"], inp["Wx"])
        x_dbl = torch.einsum("kbld,kwd->kblw", inp["xc"], inp["Wx"]).reshape(P.shape).bfloat16().float()
        rep.add_elementwise("x_dbl", x_dbl, P, bound)
        par = [inp[k] for k in ("Wdt", "bdt", "A_log")]
        rep.add("y", S.scan(inp["xc"], x_dbl, *par)[0], S.scan(inp["xc"].double(), x_dbl.double(), *[t.double() for t in par])[0], S.TOL_Y, 2)
        return
    cc = G.bwd_chunk_channels(c)
    ref, emu = S.reference(inp, chunk_channels=cc), S.reference(inp, torch.float32, chunk_channels=cc)
    if c["kind"] == "fold":
        total, bound = G.fold_bound(inp, ref, c["dt"] == "bf16")
        B, Lc, d = c["B"], c["Lc"], c["d"]
        sl = emu["slices"].bfloat16().float() if c["dt"] == "bf16" else emu["slices"]
        prod = torch.einsum("cmw,wd->cmd", sl[:, 0], inp["Wx"][0]), torch.einsum("cmw,wd->cmd", sl[:, 1], inp["Wx"][1])
        prod = torch.stack(prod, 1)                                                        # (chunk, 2, M, d)
        if c["dt"] == "bf16":                                                              # the other chunk's half is stored in bf16
            prod[0, ..., 192:], prod[1, ..., :192] = prod[0, ..., 192:].bfloat16().float(), prod[1, ..., :192].bfloat16().float()
        rep.add_elementwise("dxc+dxc2", emu["du"].reshape(2, B * Lc, d) + prod.sum(0), total, bound)
        rep.add("dx_dbl", emu["slices"], ref["slices"], S.TOL_DXDBL, 1)
        rep.add("rows", S.group_rows(emu["rows"], c["nbb"]), S.group_rows(ref["rows"], c["nbb"]), S.TOL_PARAM, 1)
        return
    S.compare_forward(rep, emu["y"], ref, emu["ckpt"])
    S.compare_backward(rep, emu["du"], emu["slices"], S.group_rows(emu["rows"], c["nbb"]), ref, nbb=c["nbb"])
    if c["kind"] == "seg":      # the segment-parallel launch writes one row per element: NBB 1 either way
        assert c["nbb"] == 1


@pytest.mark.parametrize("kind", ["short", "chunked", "seg", "generic", "fused", "fold"])
def test_fp32_emulation_stays_inside_every_bound_on_every_case(kind):
    """Were a bound tighter than plain fp32 arithmetic of the same recurrence achieves on a case's inputs, the case's
    inputs would have to change -- never the bound."""
    rep = S.Report()
    for c in G.CASES:
        if c["kind"] == kind:
            one = S.Report()
            _emulate(c, one)
            one.check(c["name"])
            for k, v in one.ratios.items():
                rep.ratios[k] = max(v, rep.ratios.get(k, 0.0))
    print(f"\nworst emulation err/bound, {kind}: " + " ".join(f"{k}={v:.3f}" for k, v in sorted(rep.ratios.items())))


# ------------------------------------------------------------------------------------------------ mutations must be noticed
@pytest.fixture(scope="module")
def mut():
    """One chunked-size shape with two channel chunks of 64, NBB 2 rows, three checkpoints; reference and emulation."""
    inp = S.make_inputs(4, 37, 72, 13, False, seed=99)
    return inp, S.reference(inp, chunk_channels=64), S.reference(inp, torch.float32, chunk_channels=64)


def _fwd_bad(y, ref, ck=None):
    rep = S.Report()
    S.compare_forward(rep, y, ref, ck)
    return rep.bad()


def _bwd_bad(emu, ref, slices=None, rows=None, nbb=2):
    rep = S.Report()
    S.compare_backward(rep, emu["du"], emu["slices"] if slices is None else slices,
                       S.group_rows(emu["rows"], nbb) if rows is None else rows, ref, nbb=nbb)
    return rep.bad()


def test_unmutated_emulation_passes(mut):
    inp, ref, emu = mut
    assert not _fwd_bad(emu["y"], ref, emu["ckpt"]) and not _bwd_bad(emu, ref)


def test_one_step_of_y_shifted_by_a_row_fails(mut):
    inp, ref, emu = mut
    y = emu["y"].clone()
    y[1, 2, 5] = emu["y"][1, 2, 6]
    assert set(_fwd_bad(y, ref)) == {"y"}


def test_direction_1_walked_ascending_fails(mut):
    inp, ref, emu = mut
    bad = S.reference(inp, torch.float32, chunk_channels=64, dir1_ascending=True)
    assert "y" in _fwd_bad(bad["y"], ref) and not _fwd_bad(torch.stack([bad["y"][0], emu["y"][1]]), ref)
    assert {"du", "dx_dbl", "rows"} <= set(_bwd_bad(bad, ref))


def test_two_swapped_dx_dbl_chunk_slices_fail(mut):
    inp, ref, emu = mut
    assert set(_bwd_bad(emu, ref, slices=emu["slices"].flip(0))) == {"dx_dbl"}
    # ... which the sum over the slices, all that was compared before, cannot see
    assert S.worst_ratio(emu["slices"].flip(0).sum(0), ref["dx_dbl"], S.TOL_DXDBL, 0) <= 1


def test_a_partial_row_covering_one_element_too_few_fails(mut):
    inp, ref, emu = mut
    rows = S.group_rows(emu["rows"], 2).clone()
    rows[1] -= emu["rows"][3]
    assert set(_bwd_bad(emu, ref, rows=rows)) == {"rows"}


def test_a_checkpoint_holding_the_previous_chunks_state_fails(mut):
    inp, ref, emu = mut
    ck = emu["ckpt"].clone()
    ck[:, :, 2] = emu["ckpt"][:, :, 1]
    assert set(_fwd_bad(emu["y"], ref, ck)) == {"ckpt"}


def test_a_dropped_weight_of_the_last_rank_quad_fails():
    inp = S.make_inputs(2, 14, 64, 49, False, seed=98)
    ref = S.reference(inp, chunk_channels=64)
    assert not _fwd_bad(S.reference(inp, torch.float32)["y"], ref)
    bad = S.reference(inp, torch.float32, chunk_channels=64, drop_rank=48)
    assert "y" in _fwd_bad(bad["y"], ref) and {"du", "dx_dbl", "rows"} <= set(_bwd_bad(bad, ref, nbb=1))


def test_one_percent_in_delta_fails(mut):
    inp, ref, emu = mut
    bad = S.reference(inp, torch.float32, chunk_channels=64, delta_scale=1.01)
    assert "y" in _fwd_bad(bad["y"], ref, bad["ckpt"]) and {"du", "dx_dbl", "rows"} <= set(_bwd_bad(bad, ref))
