"""Projection weights streamed in MFMA fragment order (mixer_ops.pack_index): the batched pack kernel against the gather
the map defines, the two fused launches on the packed copy BIT FOR BIT against the same launches on the plain weight
(only the address of a load differs, so every output -- the per-workgroup partial rows included -- is identical), and the
flat training state's packed shadows: kept current, used by the training step without changing one bit of it, and never
left behind on a model."""
import copy
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

D_IN, D = 384, 192


def _random_bf16_bits(shape, seed):
    """Random bf16 BIT PATTERNS (NaNs, infinities and denormals included): a permutation copy must move them all."""
    g = torch.Generator().manual_seed(seed)
    bits = torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int32).to(torch.int16)
    return bits.cuda().view(torch.bfloat16)


@pytest.mark.parametrize("K", [384, 768])
@pytest.mark.parametrize("njobs", [1, 24])
def test_pack_kernel_equals_the_gather_of_pack_index(K, njobs):
    from fastvim_amd import mixer_ops as M
    srcs = [_random_bf16_bits((192, K), seed=100 * njobs + K + j) for j in range(njobs)]
    dsts = [torch.zeros(192 * K, device="cuda", dtype=torch.bfloat16) for _ in range(njobs)]
    M.pack_weight_frags(srcs, dsts)
    torch.cuda.synchronize()
    for s, d_ in zip(srcs, dsts):
        ref = M.pack_weight_frags_ref(s.view(torch.int16))
        assert torch.equal(d_.view(torch.int16), ref.reshape(-1))


def _bwd_inputs(B, rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    L = rows * cols
    dev = "cuda"
    return dict(
        xz=rn(B, L, 2 * D_IN).to(dev, torch.bfloat16), d_o=rn(B, L, D_IN).to(dev, torch.bfloat16),
        dxc=rn(2, B, rows, D_IN).to(dev), dxc2=rn(2, B, rows, D_IN).to(dev, torch.bfloat16),
        dz=rn(B, L, D_IN).to(dev, torch.bfloat16),
        cw=(0.5 * rn(D_IN, 4)).to(dev), cb=(0.1 * rn(D_IN)).to(dev), cwb=(0.5 * rn(D_IN, 4)).to(dev), cbb=(0.1 * rn(D_IN)).to(dev),
        D=(1 + 0.1 * rn(D_IN)).to(dev), Db=(1 + 0.1 * rn(D_IN)).to(dev),
        W_in=(rn(2 * D_IN, D) * D ** -0.5).to(dev, torch.bfloat16), W_out=(rn(D, D_IN) * D_IN ** -0.5).to(dev, torch.bfloat16),
        gg=rn(B * L, D).to(dev), r=rn(B * L, D).to(dev), rstd=(0.5 + torch.rand(B * L, generator=g)).to(dev),
        nw=(1 + 0.1 * rn(D)).to(dev), scale=((torch.rand(B, generator=g) > 0.3).float() / 0.7).to(dev))


def _bwd_launch(t, W, packed, B, rows, cols, transposed, dxc2, sc, gg, W2):
    """The raw launch (plain or _pk entry point) into NaN-filled buffers; returns every buffer it writes."""
    from fastvim_amd import _lib as L_
    lib = L_.lib()
    Mrows, rps = B * rows * cols, rows * cols
    s_i, s_j = (1, rows) if transposed else (cols, 1)
    nan = float("nan")
    dxz = torch.full((B, rps, 2 * D_IN), nan, device="cuda", dtype=torch.bfloat16)
    dxz[:, :, D_IN:] = t["dz"]
    nb = lib.fv_mixer_conv_pool_bwd_dgrad_blocks(L_.i32(B), L_.i32(rows))
    part = torch.full((nb, 12 * D_IN), nan, device="cuda")
    dx = torch.full((Mrows, D), nan, device="cuda", dtype=torch.bfloat16)
    dri = torch.full((Mrows, D), nan, device="cuda")
    pw = torch.full((nb, D), nan, device="cuda")
    dg = torch.full((Mrows, D_IN), nan, device="cuda", dtype=torch.bfloat16) if W2 is not None else None
    fn = lib.fv_mixer_conv_pool_bwd_dgrad_pk if packed else lib.fv_mixer_conv_pool_bwd_dgrad
    rc = fn(L_.ptr(t["xz"]), L_.ptr(t["d_o"]), L_.ptr(t["dxc"]), L_.ptr(dxc2), L_.ptr(t["cw"]), L_.ptr(t["cb"]), L_.ptr(t["cwb"]),
            L_.ptr(t["cbb"]), L_.ptr(t["D"]), L_.ptr(t["Db"]), L_.ptr(dxz), L_.ptr(part), L_.i32(B), L_.i32(rows), L_.i32(cols),
            L_.i32(s_i), L_.i32(s_j), ctypes.c_float(1.0), L_.ptr(W), ctypes.c_long(2 * D_IN), L_.ptr(gg), L_.ptr(t["r"]),
            L_.ptr(t["rstd"]), L_.ptr(t["nw"]), L_.ptr(sc), L_.i32(rps), L_.ptr(dx), L_.ptr(dri), L_.ptr(pw), L_.ptr(W2), L_.ptr(dg),
            L_.i32(D_IN if W2 is not None else 0), ctypes.c_long(D_IN), L_.stream_of(dxz))
    L_.check(rc, "mixer_conv_pool_bwd_dgrad" + ("_pk" if packed else ""))
    torch.cuda.synchronize()
    return dict(dxz=dxz, part=part, dx=dx, dres_in=dri, pw=pw, dg=dg)


def _same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    v = torch.int16 if a.element_size() == 2 else torch.int32
    return torch.equal(a.view(v), b.view(v))


# geometries and option sets of tests/test_convpool_dgrad_gpu.py
@pytest.mark.parametrize("B,rows,cols,transposed", [(8, 14, 14, False), (8, 14, 14, True), (3, 14, 14, True), (5, 16, 16, False),
                                                    (5, 16, 16, True), (2, 14, 16, False), (2, 16, 14, True), (128, 14, 14, True)])
@pytest.mark.parametrize("x2,with_scale,with_gg,second", [(True, True, True, True), (False, False, False, False), (True, False, True, False)])
def test_backward_launch_packed_equals_plain(B, rows, cols, transposed, x2, with_scale, with_gg, second):
    from fastvim_amd import mixer_ops as M
    t = _bwd_inputs(B, rows, cols, seed=B + rows + 3 * int(transposed))
    W_in_t = t["W_in"].t().contiguous()
    W_pk = torch.empty(D * 2 * D_IN, device="cuda", dtype=torch.bfloat16)
    M.pack_weight_frags([W_in_t], [W_pk])
    args = (B, rows, cols, transposed, t["dxc2"] if x2 else None, t["scale"] if with_scale else None,
            t["gg"] if with_gg else None, t["W_out"] if second else None)
    plain = _bwd_launch(t, W_in_t, False, *args)
    packed = _bwd_launch(t, W_pk, True, *args)
    assert torch.isfinite(plain["dx"].float()).all() and torch.isfinite(plain["dxz"].float()).all()
    for k in plain:
        assert _same_bits(packed[k], plain[k]), k
    # ... and through the wrapper's keyword
    dxz = torch.empty_like(plain["dxz"])
    dxz[:, :, D_IN:] = t["dz"]
    p2, dx, dri, pw, nb, dg = M.conv_pool_bwd_dgrad(
        t["xz"], t["d_o"], t["dxc"], args[4], t["cw"], t["cb"], t["cwb"], t["cbb"], t["D"], t["Db"], dxz, rows, cols, transposed,
        1.0, W_in_t, args[6], t["r"], t["rstd"], t["nw"], args[5], rows * cols, W2=args[7], W_in_pk=W_pk)
    torch.cuda.synchronize()
    assert _same_bits(dx, plain["dx"]) and _same_bits(dri, plain["dres_in"]) and _same_bits(pw, plain["pw"])
    assert _same_bits(dxz, plain["dxz"]) and _same_bits(dg, plain["dg"])


def _fwd_inputs(B, rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    L = rows * cols
    dev = "cuda"
    return dict(
        xz=rn(B, L, 2 * D_IN).to(dev, torch.bfloat16), skip=rn(B, L, D_IN).to(dev, torch.bfloat16),
        yc=rn(2, B, rows, D_IN).to(dev), ln_w=(1 + 0.1 * rn(D_IN)).to(dev), ln_b=(0.1 * rn(D_IN)).to(dev),
        W=(rn(D, D_IN) * D_IN ** -0.5).to(dev, torch.bfloat16), res=rn(B * L, D).to(dev), nw=(1 + 0.1 * rn(D)).to(dev),
        scale=((torch.rand(B, generator=g) > 0.3).float() / 0.7).to(dev))


# geometries and option sets of tests/test_combine_gemm_gpu.py
@pytest.mark.parametrize("B,rows,cols,transposed", [(8, 14, 14, False), (8, 14, 14, True), (3, 14, 14, False), (3, 14, 14, True),
                                                    (5, 16, 16, True), (2, 7, 9, False), (2, 7, 9, True), (128, 14, 14, True)])
@pytest.mark.parametrize("with_ln,with_scale", [(True, True), (False, False)])
def test_forward_launch_packed_equals_plain(B, rows, cols, transposed, with_ln, with_scale):
    from fastvim_amd import mixer_ops as M
    t = _fwd_inputs(B, rows, cols, seed=B + rows + 3 * int(transposed))
    lw, lb = (t["ln_w"], t["ln_b"]) if with_ln else (None, None)
    sc = t["scale"] if with_scale else None
    W_pk = torch.empty(D * D_IN, device="cuda", dtype=torch.bfloat16)
    M.pack_weight_frags([t["W"]], [W_pk])
    res = []
    for pk in (None, W_pk):
        out = M.combine_buffers(t["xz"], lw)
        for b_ in out:
            if b_ is not None:
                b_.fill_(float("nan"))
        y, ro, rs = M.combine_out_proj_addnorm(t["xz"], t["skip"], t["yc"], lw, lb, 1e-5, rows, cols, transposed, out, t["W"],
                                               t["res"], t["nw"], sc, rows * cols, 1e-5, W_out_pk=pk)
        torch.cuda.synchronize()
        res.append((y, ro, rs) + tuple(out))
    assert torch.isfinite(res[0][0].float()).all() and torch.isfinite(res[0][1]).all()
    for a, b in zip(res[0], res[1]):
        assert _same_bits(a, b)


def _model(depth=4, classes=20, drop_path=0.1):
    from fastvim_amd.fastvim import VisionMamba
    torch.manual_seed(0)
    return VisionMamba(img_size=224, depth=depth, embed_dim=192, num_classes=classes, rms_norm=True, residual_in_fp32=True,
                       fused_add_norm=True, final_pool_type="mean", if_abs_pos_embed=True, drop_path_rate=drop_path).cuda().train()


def _packed_params(m):
    out = []
    for layer in m.layers:
        out.append((layer.mixer.in_proj.weight, True))
        out.append((layer.mixer.out_proj.weight, False))
    return out


def _assert_packed_current(m):
    """Every packed shadow is pack(current bf16 shadow), and that shadow is the bf16 cast of the fp32 master."""
    from fastvim_amd.mixer_ops import pack_weight_frags_ref
    torch.cuda.synchronize()
    for w, is_in in _packed_params(m):
        sh = w._fv_shadow
        assert torch.equal(sh, w.detach().to(torch.bfloat16))
        plain = sh.t().contiguous() if is_in else sh
        if is_in:
            assert torch.equal(w._fv_shadow_t, plain)
        assert torch.equal(w._fv_shadow_pk.view(torch.int16), pack_weight_frags_ref(plain.view(torch.int16)).reshape(-1))


def _train_step(m, flat, opt, x, tgt):
    flat.zero_grad()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = (m(x).float() * tgt).sum()
    loss.backward()
    flat.finish_backward()
    grad = flat.grad_flat.clone()
    opt.step()
    torch.cuda.synchronize()
    return loss.detach().clone(), grad


def test_flat_state_keeps_the_packed_shadows_current():
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    m = _model()
    x = torch.randn(8, 3, 224, 224, device="cuda")
    tgt = torch.randn(8, 20, device="cuda")
    with FlatTrainingState(m) as flat:
        opt = FlatAdamW(flat, m, lr=1e-2, weight_decay=0.05)
        assert all(hasattr(w, "_fv_shadow_pk") for w, _ in _packed_params(m))
        _assert_packed_current(m)
        before = m.layers[1].mixer.in_proj.weight._fv_shadow_pk.clone()
        _train_step(m, flat, opt, x, tgt)
        _assert_packed_current(m)                                   # after an optimizer step
        assert not torch.equal(before, m.layers[1].mixer.in_proj.weight._fv_shadow_pk)
        with torch.no_grad():                                       # after an in-place write: caught at the next use
            m.layers[2].mixer.in_proj.weight.mul_(0.5)
            m.layers[1].mixer.out_proj.weight.add_(0.25)
        loss, _ = _train_step(m, flat, opt, x, tgt)
        assert torch.isfinite(loss)
        _assert_packed_current(m)
        with torch.no_grad():                                       # ... re-packed by that use itself, before any optimizer step
            m.layers[2].mixer.in_proj.weight.mul_(2.0)
            m.layers[1].mixer.out_proj.weight.sub_(0.125)
        flat.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            (m(x).float() * tgt).sum().backward()
        flat.finish_backward()
        _assert_packed_current(m)
        sd = {k: (v * 0.75 if v.is_floating_point() else v) for k, v in m.state_dict().items()}
        m.load_state_dict(sd)                                       # after load_state_dict (post hook)
        _assert_packed_current(m)


def test_training_step_is_bit_identical_with_and_without_the_packed_path(monkeypatch):
    from fastvim_amd import mamba_simple_faster as msf
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    base = _model()
    x = torch.randn(32, 3, 224, 224, device="cuda")
    tgt = torch.randn(32, 20, device="cuda")
    res = []
    for on in (True, False):
        m = copy.deepcopy(base)
        calls = {"fwd": 0, "bwd": 0}
        real_f, real_b = msf.M.combine_out_proj_addnorm, msf.M.conv_pool_bwd_dgrad
        monkeypatch.setattr(msf.M, "combine_out_proj_addnorm",
                            lambda *a, **k: (calls.__setitem__("fwd", calls["fwd"] + (k.get("W_out_pk") is not None)), real_f(*a, **k))[1])
        monkeypatch.setattr(msf.M, "conv_pool_bwd_dgrad",
                            lambda *a, **k: (calls.__setitem__("bwd", calls["bwd"] + (k.get("W_in_pk") is not None)), real_b(*a, **k))[1])
        was = msf.use_packed_weights(on)
        try:
            with FlatTrainingState(m) as flat:
                opt = FlatAdamW(flat, m, lr=1e-2, weight_decay=0.05)
                out = []
                for _ in range(2):
                    torch.manual_seed(7)
                    out.append(_train_step(m, flat, opt, x, tgt))
                res.append((out, flat.param_flat.clone(), flat.shadow_flat.clone()))
        finally:
            msf.use_packed_weights(was)
            monkeypatch.setattr(msf.M, "combine_out_proj_addnorm", real_f)
            monkeypatch.setattr(msf.M, "conv_pool_bwd_dgrad", real_b)
        if on:
            assert calls["fwd"] > 0 and calls["bwd"] > 0, calls      # the packed launches were really taken
        else:
            assert calls["fwd"] == 0 and calls["bwd"] == 0, calls
    for (l1, g1), (l0, g0) in zip(res[0][0], res[1][0]):
        assert torch.equal(l1, l0) and torch.equal(g1, g0)
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])


def test_graph_replay_equals_eager_with_the_packed_path():
    import fastvim_amd
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    from fastvim_amd.pipeline import SegmentedTrainStep
    if not fastvim_amd.graph_capture_safe():
        pytest.skip("HIP graph capture is not safe in this process")
    base = _model(drop_path=0.0)
    x = torch.randn(16, 3, 224, 224, device="cuda")
    tgt = torch.randn(16, 20, device="cuda")
    res = []
    for use_graph in (True, False):
        m = copy.deepcopy(base)
        with FlatTrainingState(m) as flat:
            opt = FlatAdamW(flat, m, lr=1e-2, weight_decay=0.05)
            step = SegmentedTrainStep(m, flat, opt, lambda lg, t_: (lg.float() * t_).sum(), x, tgt, n_segments=1, use_graph=use_graph)
            assert step.use_graph == use_graph
            losses = []
            for _ in range(3):
                losses.append(step.step().clone())
            torch.cuda.synchronize()
            _assert_packed_current(m)
            res.append((torch.stack(losses), flat.param_flat.clone(), flat.grad_flat.clone()))
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)


def test_no_derived_shadow_survives_close_or_a_second_state():
    from fastvim_amd.flat import FlatTrainingState
    m = _model(depth=2)
    attrs = ("_fv_shadow_t", "_fv_shadow_t_version", "_fv_shadow_pk", "_fv_shadow_pk_version")

    def leftovers():
        found = [(n, a) for n, p in m.named_parameters() for a in attrs if hasattr(p, a)]
        for name, mod in m.named_modules():
            fv = mod.__dict__.get("_fv")
            if isinstance(fv, dict):
                found += [(name, k) for k in ("Wx2_shadow_t", "Wx2_t_params") if k in fv]
        return found

    flat = FlatTrainingState(m)
    assert any(a == "_fv_shadow_pk" for _, a in leftovers()) and any(a == "_fv_shadow_t" for _, a in leftovers())
    flat.close()
    assert leftovers() == []
    flat = FlatTrainingState(m)                                      # a bf16 state that is never closed ...
    assert leftovers() != []
    flat2 = FlatTrainingState(m, shadow_dtype=torch.float32)         # ... then one that keeps no bf16 copies: nothing stale is left
    assert leftovers() == []
    flat2.close()
    assert leftovers() == []
