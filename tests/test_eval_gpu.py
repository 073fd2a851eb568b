"""The validation step on the GPU: the swap kernel bit for bit, the metric kernels against the fp64 reference of
``eval_ref.py`` and against ``fv_label_ce``'s own rows, and ``ValidationStep`` on the small model of
tests/test_pipeline_gpu.py -- graph against eager, the live half against the plain evaluation forward, the EMA half
against EMA weights put in by hand, and the training trajectory around it bit for bit."""
import ctypes

import pytest
import torch

import eval_ref as R

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------- swap kernel
def _swap(p, e, s):
    from fastvim_amd import _lib as L
    rc = L.lib().fv_swap_params_ema(L.ptr(p), L.ptr(e), L.ptr(s), L.i32(L.dtype_code(s.dtype)), ctypes.c_size_t(p.numel()),
                                    L.stream_of(p))
    L.check(rc, "swap_params_ema")


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _special_bits():
    """fp32 bit patterns: +-0, +-inf, denormals (largest, smallest, one in between), and values exactly half way between
    two bf16 neighbours (low half 0x8000: round-to-nearest-even goes down after an even mantissa, up after an odd one,
    and from the largest finite bf16 to infinity)."""
    pats = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x007FFFFF, 0x00000001, 0x80012345, 0x00008000, 0x00018000,
            0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x7F7F8000, 0x3F807FFF, 0x3F808001]
    return torch.tensor([v - 2 ** 32 if v >= 2 ** 31 else v for v in pats], dtype=torch.int32)


def _values(n, seed):
    g = torch.Generator().manual_seed(seed)
    bits = (torch.randn(n, generator=g) * 3).view(torch.int32).clone()
    tie = torch.rand(n, generator=g) < 0.125                                 # one in eight lands on a rounding tie
    bits[tie] = (bits[tie] & -65536) | 0x8000
    sp = torch.roll(_special_bits(), seed)
    k = min(n, sp.numel())
    bits[torch.randperm(n, generator=g)[:k]] = sp[:k]
    x = bits.view(torch.float32)
    assert not bool(torch.isnan(x).any())
    return x


GUARD = 8


def _guarded(values, dtype, offset):
    """``values`` as a view ``offset`` elements into a fresh allocation, with guard elements on both sides."""
    n = values.numel()
    base = torch.full((GUARD + offset + n + GUARD,), 7.0, device="cuda", dtype=dtype)
    view = base[GUARD + offset:GUARD + offset + n]
    view.copy_(values)
    return base, view


def _guards_intact(base, view_len, offset):
    lo, hi = base[:GUARD + offset], base[GUARD + offset + view_len:]
    return bool((lo == 7.0).all()) and bool((hi == 7.0).all())


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 4, 1023, 4099, 2 ** 20 + 5])
def test_swap_exchanges_bit_for_bit(n, offset):
    """offset 1: views one element into their allocations -- 4-byte aligned fp32, 2-byte aligned bf16."""
    p0, e0 = _values(n, 1 + n % 7).cuda(), _values(n, 11 + n % 5).cuda()
    pb, p = _guarded(p0, torch.float32, offset)
    eb, e = _guarded(e0, torch.float32, offset)
    sb, s = _guarded(p0.to(torch.bfloat16), torch.bfloat16, offset)
    s0 = s.clone()
    assert p.data_ptr() % 16 == (4 * offset) % 16 and s.data_ptr() % 8 == (2 * offset) % 8
    _swap(p, e, s)
    assert torch.equal(_bits(p), _bits(e0)) and torch.equal(_bits(e), _bits(p0))
    assert torch.equal(_bits(s), _bits(e0.to(torch.bfloat16)))
    _swap(p, e, s)
    assert torch.equal(_bits(p), _bits(p0)) and torch.equal(_bits(e), _bits(e0)) and torch.equal(_bits(s), _bits(s0))
    for base in (pb, eb, sb):
        assert _guards_intact(base, n, offset)


def test_swap_rounds_ties_and_denormals_like_torch():
    """Every special pattern on its own, so that none can hide behind another: shadow == torch's fp32 -> bf16 cast."""
    x = _special_bits().view(torch.float32).cuda()
    p, e, s = torch.zeros_like(x), x.clone(), torch.zeros(x.numel(), device="cuda", dtype=torch.bfloat16)
    _swap(p, e, s)
    want = x.to(torch.bfloat16)
    assert torch.equal(_bits(s), _bits(want)), (_bits(s).tolist(), _bits(want).tolist())
    w = [v & 0xFFFF for v in _bits(want).tolist()]
    # torch's cast, the reference: a denormal stays one, ties go to the even neighbour, the tie above the largest finite to inf
    assert (w[6], w[7], w[8], w[9], w[10], w[13]) == (0x8001, 0x0000, 0x0002, 0x3F80, 0x3F82, 0x7F80)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_swap_other_shadow_dtypes(dtype):
    n = 4099
    p0, e0 = _values(n, 3).cuda(), _values(n, 4).cuda()
    p, e, s = p0.clone(), e0.clone(), torch.zeros(n, device="cuda", dtype=dtype)
    _swap(p, e, s)
    assert torch.equal(_bits(p), _bits(e0)) and torch.equal(_bits(e), _bits(p0)) and torch.equal(_bits(s), _bits(e0.to(dtype)))


def test_swap_with_unequal_offsets_takes_the_element_path():
    """param one element in, ema and the shadow at the start of theirs: no common 16-byte phase."""
    n = 4099
    p0, e0 = _values(n, 5).cuda(), _values(n, 6).cuda()
    pb, p = _guarded(p0, torch.float32, 1)
    eb, e = _guarded(e0, torch.float32, 0)
    sb, s = _guarded(p0.to(torch.bfloat16), torch.bfloat16, 0)
    _swap(p, e, s)
    assert torch.equal(_bits(p), _bits(e0)) and torch.equal(_bits(e), _bits(p0)) and torch.equal(_bits(s), _bits(e0.to(torch.bfloat16)))
    assert _guards_intact(pb, n, 1) and _guards_intact(eb, n, 0) and _guards_intact(sb, n, 0)


def test_swap_keeps_nan_a_nan():
    """NaNs with payloads, quiet and signalling: the fp32 buffers exchange their bits; the shadow is a NaN where the new
    parameter is one (the payload is not compared)."""
    n = 1023
    p0, e0 = _values(n, 8), _values(n, 9)
    nan_bits = torch.tensor([0x7FC00000, 0x7F800001, 0x7FFFFFFF, -0x003EDCBB], dtype=torch.int32)      # (the last: 0xFFC12345)
    _bits(e0)[[0, 5, 500, 1022]] = nan_bits
    _bits(p0)[[1, 6]] = nan_bits[:2]
    p0, e0 = p0.cuda(), e0.cuda()
    p, e, s = p0.clone(), e0.clone(), torch.zeros(n, device="cuda", dtype=torch.bfloat16)
    _swap(p, e, s)
    assert torch.equal(_bits(p), _bits(e0)) and torch.equal(_bits(e), _bits(p0))
    assert torch.equal(torch.isnan(s), torch.isnan(e0)) and int(torch.isnan(s).sum()) == 4
    ok = ~torch.isnan(e0)
    assert torch.equal(_bits(s)[ok], _bits(e0.to(torch.bfloat16))[ok])
    _swap(p, e, s)
    assert torch.equal(_bits(p), _bits(p0)) and torch.equal(_bits(e), _bits(e0))
    assert torch.equal(torch.isnan(s), torch.isnan(p0)) and int(torch.isnan(s).sum()) == 2


# ---------------------------------------------------------------------------------------------------- metric kernels
def _label_ce_rows(x, labels):
    """loss_rows / correct_rows of fv_label_ce(mix = NULL, smoothing = 0) on the given rows."""
    from fastvim_amd import _lib as L
    B, C = x.shape
    rows = torch.empty(B, device="cuda", dtype=torch.float32)
    loss = torch.empty(1, device="cuda", dtype=torch.float32)
    corr = torch.empty(B, device="cuda", dtype=torch.int32)
    ncorr = torch.empty(1, device="cuda", dtype=torch.int32)
    x, labels = x.contiguous(), labels.contiguous()
    rc = L.lib().fv_label_ce(L.ptr(x), L.i32(L.dtype_code(x.dtype)), L.ptr(labels), L.ptr(None), ctypes.c_double(0.0),
                             L.ptr(rows), L.ptr(loss), L.ptr(None), L.ptr(corr), L.ptr(ncorr), L.i32(B), L.i32(C), L.stream_of(x))
    L.check(rc, "label_ce")
    return rows, corr


def _check_block(block, ref, rows_sum=None):
    got = R.unpack_block(block)
    assert got["n"] == ref["n"] and got["n_correct"] == ref["n_correct"]
    assert torch.equal(got["support"], ref["support"]) and torch.equal(got["hit"], ref["hit"])
    n = ref["n"]
    print(f"loss_sum {got['loss_sum']!r} reference {ref['loss_sum']!r} sum of fv_label_ce rows {rows_sum!r} n {n}")
    if rows_sum is not None:
        assert abs(got["loss_sum"] - rows_sum) <= 1e-12 * abs(rows_sum)
    if n:
        want = ref["loss_sum"] / n
        assert abs(got["loss_sum"] / n - want) <= 2e-5 * max(1.0, abs(want))
    else:
        assert got["loss_sum"] == 0.0
    return got


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,C", [(1, 2), (5, 10), (4, 1000), (130, 1000), (5, 2048)])
def test_accumulate_vs_reference(B, C, dtype):
    from fastvim_amd.evaluate import EvalMetrics
    for nv in sorted({1, B - 1, B}):
        x, y = R.make_batch(B, C, dtype, nv, seed=B * 7 + C + nv, device="cuda")
        m = EvalMetrics(C, "cuda")
        m.update(x, y, n_valid=nv)
        ref = R.reference(x, y, nv, C)
        rows_sum = None
        if nv:
            rows, corr = _label_ce_rows(x[:nv], y[:nv])
            got_rows, got_corr = m.scratch(B)
            assert torch.equal(_bits(got_rows[:nv]), _bits(rows)) and torch.equal(got_corr[:nv], corr)      # the same bits
            assert not bool(got_rows[nv:].any()) and not bool(got_corr[nv:].any())
            rows_sum = float(rows.double().sum())
            assert 0 < ref["n_correct"] < nv or nv < 100
        _check_block(m.block, ref, rows_sum)
        out = m.compute()
        assert out["n"] == nv and (nv == 0 or out["acc_micro"] == ref["n_correct"] / nv)


def test_three_updates_reset_and_determinism():
    from fastvim_amd.evaluate import EvalMetrics
    B, C = 130, 1000
    batches = [R.make_batch(B, C, torch.bfloat16, nv, seed=40 + i, device="cuda") + (nv,) for i, nv in enumerate((130, 77, 1))]

    def run():
        m = EvalMetrics(C, "cuda")
        for x, y, nv in batches:
            m.update(x, y, n_valid=nv)
        return m
    m1, m2 = run(), run()
    ref = R.merge([R.reference(x, y, nv, C) for x, y, nv in batches])
    _check_block(m1.block, ref)
    assert torch.equal(m1.block, m2.block)                                   # two identical runs: the same bytes
    out = m1.compute()
    assert out["n"] == 208 and out["acc_micro"] == ref["n_correct"] / 208
    present = ref["support"] > 0
    want_macro = float((ref["hit"][present].double() / ref["support"][present].double()).mean())
    assert out["acc_macro"] == pytest.approx(want_macro, rel=1e-15)
    # n_valid = 0 changes nothing
    before = m1.block.clone()
    m1.update(*batches[0][:2], n_valid=0)
    assert torch.equal(m1.block, before)
    m1.reset()
    assert not bool(m1.block.any())
    m1.update(*batches[2][:2], n_valid=1)                                    # ... and the block counts from zero again
    assert R.unpack_block(m1.block)["n"] == 1


def test_out_of_range_label_is_seen_and_counted_nowhere():
    """Valid rows with label C, a huge one and a negative one; the words around the class counters are watched."""
    from fastvim_amd.evaluate import EvalMetrics
    B, C = 6, 10
    x, y = R.make_batch(B, C, torch.float32, 5, seed=5, device="cuda")
    y[1], y[2], y[3] = C, 2 ** 40, -3
    m = EvalMetrics(C, "cuda")
    m.update(x, y, n_valid=5)
    ref = R.reference(x, y, 5, C)
    got = _check_block(m.block, ref)
    assert got["n"] == 5 and int(got["support"].sum()) == 2 and got["n_correct"] <= 2
    rows, corr = m.scratch(B)
    assert rows[1:4].tolist() == [0.0, 0.0, 0.0] and corr[1:4].tolist() == [0, 0, 0]


# ---------------------------------------------------------------------------------------------------- ValidationStep
BATCH, CLASSES = 4, 100
N_VALID = (4, 4, 3)


def _make(ema_decay=0.999):
    from fastvim_amd.fastvim import VisionMamba
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    torch.manual_seed(0)
    m = VisionMamba(img_size=224, depth=4, embed_dim=192, num_classes=CLASSES, rms_norm=True, residual_in_fp32=True,
                    fused_add_norm=True, final_pool_type="mean", if_abs_pos_embed=True, drop_path_rate=0.1).cuda().train()
    flat = FlatTrainingState(m)
    nd = {n for n, p in m.named_parameters() if p.ndim <= 1 or n.endswith(".bias") or n in m.no_weight_decay()}
    return m, flat, FlatAdamW(flat, m, lr=1e-3, weight_decay=0.05, no_decay=nd, ema_decay=ema_decay)


def _train(m, flat, opt, x, y, steps):
    from fastvim_amd.losses import CrossEntropyLoss
    crit, losses = CrossEntropyLoss(), []
    for _ in range(steps):
        flat.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = crit(m(x), y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return losses


def _state_tensors(flat, opt):
    out = {"param_flat": flat.param_flat, "ema": opt.ema, "shadow_flat": flat.shadow_flat, "grad_flat": flat.grad_flat,
           "exp_avg": opt.exp_avg, "exp_avg_sq": opt.exp_avg_sq, "step_t": opt.step_t, "lr": opt.lr}
    for name in ("_t_dst", "_tx_dst", "_pk_dst"):
        for i, t in enumerate(getattr(flat, name, [])):
            out[f"{name}[{i}]"] = t
    return out


def _val_batches():
    g = torch.Generator().manual_seed(123)
    out = []
    for nv in N_VALID:
        x = torch.randn(BATCH, 3, 224, 224, generator=g)
        y = torch.randint(0, CLASSES, (BATCH,), generator=g)
        x[nv:] = 1.0e3 * torch.randn(BATCH - nv, 3, 224, 224, generator=g)          # the rows of a short batch: garbage
        y[nv:] = -1
        out.append((x.cuda(), y.cuda(), nv))
    return out


@pytest.fixture(scope="module")
def runs():
    """ONE trained state, validated by a graph step and by an eager step over the same three batches (the last one
    short), then once more with the EMA weights put in by hand; the tests below look at what it recorded."""
    from fastvim_amd.evaluate import ValidationStep
    from fastvim_amd.losses import CrossEntropyLoss
    r = {}
    m, flat, opt = _make()
    torch.manual_seed(7)
    xt, yt = torch.randn(BATCH, 3, 224, 224, device="cuda"), torch.randint(0, CLASSES, (BATCH,), device="cuda")
    _train(m, flat, opt, xt, yt, 3)
    assert not torch.equal(opt.ema, flat.param_flat)
    state = _state_tensors(flat, opt)
    assert any(k.startswith("_t_dst") for k in state) and any(k.startswith("_pk_dst") for k in state)
    before = {k: v.clone() for k, v in state.items()}
    rng = (torch.get_rng_state(), torch.cuda.get_rng_state())
    xv = torch.zeros(BATCH, 3, 224, 224, device="cuda")
    yv = torch.zeros(BATCH, dtype=torch.int64, device="cuda")
    vg = ValidationStep(m, flat, opt, xv, yv)
    ve = ValidationStep(m, flat, opt, xv, yv, use_graph=False)
    r["graph_captured"] = vg.graph is not None
    r["training_after_construction"] = m.training and all(mod.training for mod in m.modules())
    batches = _val_batches()
    for x, y, nv in batches:
        xv.copy_(x); yv.copy_(y)
        vg.step(n_valid=nv)
        ve.step(n_valid=nv)
    torch.cuda.synchronize()
    r["training_after_steps"] = m.training and all(mod.training for mod in m.modules())
    r["rng_unchanged"] = torch.equal(rng[0], torch.get_rng_state()) and torch.equal(rng[1], torch.cuda.get_rng_state())
    r["state_changed"] = [k for k, v in state.items() if not torch.equal(_bits(v), _bits(before[k]))]
    r["graph"] = (vg.live.block.clone(), vg.ema_metrics.block.clone())
    r["eager"] = (ve.live.block.clone(), ve.ema_metrics.block.clone())
    r["compute"] = vg.compute()
    # the plain way: evaluation forward of every batch, loss and count of its valid rows, summed on the host
    crit = CrossEntropyLoss()
    host = {"loss_sum": 0.0, "n": 0, "n_correct": 0, "refs": []}
    m.eval()
    for x, y, nv in batches:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            logits = m(x)
        loss, nc = crit.loss_and_correct(logits[:nv].contiguous(), y[:nv].contiguous())
        host["loss_sum"] += loss.double().item() * nv
        host["n"] += nv
        host["n_correct"] += int(nc.item())
        host["refs"].append(R.reference(logits, y, nv, CLASSES))
    m.train()
    r["host"] = host
    # the EMA weights put in by hand, validated as live weights
    keep = flat.param_flat.clone()
    with torch.no_grad():
        flat.param_flat.copy_(opt.ema)
    flat.refresh_shadow()
    flat.refresh_transposed()
    vh = ValidationStep(m, flat, opt, xv, yv, ema=False)
    for x, y, nv in batches:
        xv.copy_(x); yv.copy_(y)
        vh.step(n_valid=nv)
    r["by_hand"] = vh.live.block.clone()
    r["by_hand_has_ema_metrics"] = vh.ema_metrics is not None
    r["by_hand_compute"] = vh.compute()
    with torch.no_grad():
        flat.param_flat.copy_(keep)
    flat.refresh_shadow()
    vg.reset()
    r["after_reset"] = (vg.live.block.clone(), vg.ema_metrics.block.clone())
    torch.cuda.synchronize()
    flat.close()
    return r


def test_graph_and_eager_leave_the_same_blocks(runs):
    assert runs["graph_captured"]
    assert torch.equal(runs["graph"][0], runs["eager"][0]) and torch.equal(runs["graph"][1], runs["eager"][1])
    assert R.unpack_block(runs["graph"][0])["n"] == sum(N_VALID)


def test_live_half_equals_the_plain_evaluation_forward(runs):
    got, host = R.unpack_block(runs["graph"][0]), runs["host"]
    ref = R.merge(host["refs"])
    print(f"live: loss_sum {got['loss_sum']!r} host {host['loss_sum']!r} fp64 reference on the logits {ref['loss_sum']!r}")
    assert got["n"] == host["n"] == sum(N_VALID) and got["n_correct"] == host["n_correct"] == ref["n_correct"]
    assert torch.equal(got["support"], ref["support"]) and torch.equal(got["hit"], ref["hit"])
    n = got["n"]
    for want in (host["loss_sum"] / n, ref["loss_sum"] / n):
        assert abs(got["loss_sum"] / n - want) <= 2e-5 * max(1.0, abs(want))
    c = runs["compute"]
    assert c["n"] == n and c["val_loss"] == got["loss_sum"] / n and c["val_acc"] == got["n_correct"] / n
    assert set(c) == {"val_loss", "val_acc", "val_acc_macro", "val_loss_ema", "val_acc_ema", "val_acc_macro_ema", "n"}


def test_ema_half_equals_ema_weights_put_in_by_hand(runs):
    """Byte for byte: any copy the swap forgets to re-make would be read by the forward and show here."""
    assert torch.equal(runs["graph"][1], runs["by_hand"])
    assert not torch.equal(runs["graph"][1], runs["graph"][0])               # ... and the two halves differ: not vacuous
    e = R.unpack_block(runs["graph"][1])
    assert e["n"] == sum(N_VALID) and runs["compute"]["val_loss_ema"] == e["loss_sum"] / e["n"]


def test_ema_false_fills_only_the_live_metrics(runs):
    assert not runs["by_hand_has_ema_metrics"]
    assert set(runs["by_hand_compute"]) == {"val_loss", "val_acc", "val_acc_macro", "n"}
    assert runs["by_hand_compute"]["n"] == sum(N_VALID)


def test_validation_leaves_the_training_state_untouched(runs):
    assert runs["state_changed"] == []
    assert runs["training_after_construction"] and runs["training_after_steps"] and runs["rng_unchanged"]


def test_short_last_batch_counts_its_valid_rows_only(runs):
    """The third batch: three valid rows, garbage and label -1 in row 3.  n over the epoch is the number of valid samples
    and the counts are those of the references over the valid rows alone."""
    got, refs = R.unpack_block(runs["graph"][0]), runs["host"]["refs"]
    assert refs[2]["n"] == 3 and got["n"] == 11 and int(got["support"].sum()) == 11
    assert got["n_correct"] == sum(r["n_correct"] for r in refs)


def test_reset_zeroes_both_blocks(runs):
    assert not bool(runs["after_reset"][0].any()) and not bool(runs["after_reset"][1].any())


def test_train_validate_train_equals_train_train():
    """DropPath on: a validation in the middle (construction, three graph steps, compute) must leave parameters, EMA and
    losses of the following training steps bit for bit what they are without it -- a transposed or packed copy not
    restored for the backward, or a disturbed RNG stream, shows here."""
    from fastvim_amd.evaluate import ValidationStep
    torch.manual_seed(3)
    xt, yt = torch.randn(BATCH, 3, 224, 224, device="cuda"), torch.randint(0, CLASSES, (BATCH,), device="cuda")
    out = []
    for validate in (False, True):
        m, flat, opt = _make()
        torch.manual_seed(11)
        losses = _train(m, flat, opt, xt, yt, 2)
        if validate:
            xv, yv = torch.randn(BATCH, 3, 224, 224, generator=torch.Generator().manual_seed(5)).cuda(), yt.clone()
            val = ValidationStep(m, flat, opt, xv, yv)
            for nv in N_VALID:
                val.step(n_valid=nv)
            assert val.compute()["n"] == sum(N_VALID)
        losses += _train(m, flat, opt, xt, yt, 2)
        out.append((losses, flat.param_flat.clone(), opt.ema.clone(), flat.shadow_flat.clone()))
        flat.close()
    (l0, p0, e0, s0), (l1, p1, e1, s1) = out
    assert l0 == l1, (l0, l1)
    assert torch.equal(p0, p1) and torch.equal(e0, e1) and torch.equal(_bits(s0), _bits(s1))


def test_ema_weights_context_and_missing_ema():
    from fastvim_amd.evaluate import ValidationStep, ema_weights
    from fastvim_amd.fastvim import VisionMamba
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    torch.manual_seed(0)
    m = VisionMamba(img_size=64, patch_size=16, depth=2, embed_dim=64, num_classes=10, rms_norm=True, residual_in_fp32=True,
                    fused_add_norm=True, final_pool_type="mean", drop_path_rate=0.0).cuda().train()
    with FlatTrainingState(m) as flat:
        x, y = torch.randn(2, 3, 64, 64, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")
        plain = FlatAdamW(flat, m, lr=1e-3)
        with pytest.raises(RuntimeError, match="ema_decay"):
            ValidationStep(m, flat, plain, x, y)
        with pytest.raises(RuntimeError, match="ema_decay"):
            plain.swap_ema_()
        v = ValidationStep(m, flat, plain, x, y, ema=False, use_graph=False)
        v.step()
        assert v.compute()["n"] == 2 and m.training
        opt = FlatAdamW(flat, m, lr=1e-3, ema_decay=0.9)
        with torch.no_grad():
            opt.ema.mul_(1.5)
        p0, e0, s0 = flat.param_flat.clone(), opt.ema.clone(), flat.shadow_flat.clone()
        with ema_weights(opt):
            assert torch.equal(flat.param_flat, e0) and torch.equal(opt.ema, p0)
            assert torch.equal(_bits(flat.shadow_flat), _bits(e0.to(torch.bfloat16)))
        assert torch.equal(flat.param_flat, p0) and torch.equal(opt.ema, e0) and torch.equal(_bits(flat.shadow_flat), _bits(s0))
