"""The second weight of the fused backward launch streamed in MFMA fragment order (mixer_ops.pack_index_w2,
fv_mixer_conv_pool_bwd_dgrad_pk2): the batched pack kernel against the gather the map defines, the launch on the packed
W_out BIT FOR BIT against the same launch on the plain W_out (same operands, k order and accumulation chains, so every
output -- the per-workgroup partial rows included -- is identical), and the flat training state's new shadow: kept current,
used by the training step without changing one bit of it, and never left behind on a model."""
import copy
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

D_IN, D = 384, 192
SENTINEL = 0x5A5B          # bf16 bit pattern d g is pre-filled with


def _random_bf16_bits(shape, seed):
    """Random bf16 BIT PATTERNS (NaNs, infinities and denormals included): a permutation copy must move them all."""
    g = torch.Generator().manual_seed(seed)
    bits = torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int32).to(torch.int16)
    return bits.cuda().view(torch.bfloat16)


@pytest.mark.parametrize("njobs", [1, 24])
def test_pack_w2_kernel_equals_the_gather_of_pack_index_w2(njobs):
    from fastvim_amd import mixer_ops as M
    srcs = [_random_bf16_bits((D, D_IN), seed=100 * njobs + j) for j in range(njobs)]
    dsts = [torch.zeros(D * D_IN, device="cuda", dtype=torch.bfloat16) for _ in range(njobs)]
    M.pack_weight_frags_w2(srcs, dsts)
    torch.cuda.synchronize()
    for s, d_ in zip(srcs, dsts):
        ref = M.pack_weight_frags_w2_ref(s.view(torch.int16))
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


def _bwd_launch(t, W_in_pk, W2, pk2, B, rows, cols, transposed, dxc2, sc, gg):
    """The raw launch (_pk or _pk2 entry point) into NaN-filled buffers; d g lies between two guard images filled with a
    sentinel, like d g itself.  Returns every buffer the launch writes, and d g with its guards."""
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
    dg_all = torch.full(((B + 2) * rps, D_IN), SENTINEL, device="cuda", dtype=torch.int16).view(torch.bfloat16)
    dg = dg_all[rps:rps + Mrows]
    fn = lib.fv_mixer_conv_pool_bwd_dgrad_pk2 if pk2 else lib.fv_mixer_conv_pool_bwd_dgrad_pk
    rc = fn(L_.ptr(t["xz"]), L_.ptr(t["d_o"]), L_.ptr(t["dxc"]), L_.ptr(dxc2), L_.ptr(t["cw"]), L_.ptr(t["cb"]), L_.ptr(t["cwb"]),
            L_.ptr(t["cbb"]), L_.ptr(t["D"]), L_.ptr(t["Db"]), L_.ptr(dxz), L_.ptr(part), L_.i32(B), L_.i32(rows), L_.i32(cols),
            L_.i32(s_i), L_.i32(s_j), ctypes.c_float(1.0), L_.ptr(W_in_pk), ctypes.c_long(2 * D_IN), L_.ptr(gg), L_.ptr(t["r"]),
            L_.ptr(t["rstd"]), L_.ptr(t["nw"]), L_.ptr(sc), L_.i32(rps), L_.ptr(dx), L_.ptr(dri), L_.ptr(pw), L_.ptr(W2), L_.ptr(dg),
            L_.i32(D_IN), ctypes.c_long(D_IN), L_.stream_of(dxz))
    L_.check(rc, "mixer_conv_pool_bwd_dgrad" + ("_pk2" if pk2 else "_pk"))
    torch.cuda.synchronize()
    return dict(dxz=dxz, part=part, dx=dx, dres_in=dri, pw=pw, dg=dg), dg_all


def _same_bits(a, b):
    v = torch.int16 if a.element_size() == 2 else torch.int32
    return torch.equal(a.view(v), b.view(v))


# 14-row grids cut 4-4-4-2 and the 6-row grid 4-2 (a last tile with waves that have no pooling row); 14-column grids
# leave dead tile rows; 16 x 16 has neither
@pytest.mark.parametrize("B,rows,cols", [(2, 14, 14), (2, 16, 16), (2, 14, 16), (2, 16, 14), (2, 6, 14)])
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("x2,with_scale,with_gg", [(True, True, True), (False, False, False)])
def test_backward_launch_packed_w2_equals_plain_w2(B, rows, cols, transposed, x2, with_scale, with_gg):
    from fastvim_amd import mixer_ops as M
    t = _bwd_inputs(B, rows, cols, seed=B + rows + 5 * cols + 3 * int(transposed))
    W_in_t = t["W_in"].t().contiguous()
    W_pk = torch.empty(D * 2 * D_IN, device="cuda", dtype=torch.bfloat16)
    M.pack_weight_frags([W_in_t], [W_pk])
    W2_pk = torch.empty(D * D_IN, device="cuda", dtype=torch.bfloat16)
    M.pack_weight_frags_w2([t["W_out"]], [W2_pk])
    args = (B, rows, cols, transposed, t["dxc2"] if x2 else None, t["scale"] if with_scale else None, t["gg"] if with_gg else None)
    plain, plain_all = _bwd_launch(t, W_pk, t["W_out"], False, *args)
    packed, packed_all = _bwd_launch(t, W_pk, W2_pk, True, *args)
    rps = rows * cols
    for k in ("dx", "dg", "dres_in", "pw", "part"):
        assert torch.isfinite(plain[k].float()).all(), k
    assert torch.isfinite(plain["dxz"][:, :, :D_IN].float()).all()
    for k in plain:                      # the x half of d xz, d x, d residual, d g, both partial-row tensors
        assert _same_bits(packed[k], plain[k]), k
    # rows of tokens outside the launch's images are untouched, every row inside is written
    for all_ in (plain_all, packed_all):
        bits = all_.view(torch.int16)
        assert (bits[:rps] == SENTINEL).all() and (bits[rps + B * rps:] == SENTINEL).all()
    # ... and through the wrapper's keyword
    dxz = torch.empty_like(plain["dxz"])
    dxz[:, :, D_IN:] = t["dz"]
    p2, dx, dri, pw, nb, dg = M.conv_pool_bwd_dgrad(
        t["xz"], t["d_o"], t["dxc"], args[4], t["cw"], t["cb"], t["cwb"], t["cbb"], t["D"], t["Db"], dxz, rows, cols, transposed,
        1.0, W_in_t, args[6], t["r"], t["rstd"], t["nw"], args[5], rps, W2=t["W_out"], W_in_pk=W_pk, W2_pk=W2_pk)
    torch.cuda.synchronize()
    assert _same_bits(dx, plain["dx"]) and _same_bits(dri, plain["dres_in"]) and _same_bits(pw, plain["pw"])
    assert _same_bits(dxz[:, :, :D_IN], plain["dxz"][:, :, :D_IN]) and _same_bits(dg, plain["dg"])


def _model(depth=3, classes=20, drop_path=0.1):
    from fastvim_amd.fastvim import VisionMamba
    torch.manual_seed(0)
    return VisionMamba(img_size=224, depth=depth, embed_dim=192, num_classes=classes, rms_norm=True, residual_in_fp32=True,
                       fused_add_norm=True, final_pool_type="mean", if_abs_pos_embed=True, drop_path_rate=drop_path).cuda().train()


def _assert_w2_current(m):
    """Every W2 shadow is pack_index_w2 of the current bf16 shadow, and that shadow is the bf16 cast of the fp32 master."""
    from fastvim_amd.mixer_ops import pack_weight_frags_w2_ref
    torch.cuda.synchronize()
    for layer in m.layers:
        w = layer.mixer.out_proj.weight
        sh = w._fv_shadow
        assert torch.equal(sh, w.detach().to(torch.bfloat16))
        assert torch.equal(w._fv_shadow_pk2.view(torch.int16), pack_weight_frags_w2_ref(sh.view(torch.int16)).reshape(-1))


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


def test_flat_state_keeps_the_w2_shadow_current_and_drops_it():
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    m = _model()
    x = torch.randn(2, 3, 224, 224, device="cuda")
    tgt = torch.randn(2, 20, device="cuda")
    attrs = ("_fv_shadow_pk2", "_fv_shadow_pk2_version")
    leftovers = lambda: [(n, a) for n, p in m.named_parameters() for a in attrs if hasattr(p, a)]
    with FlatTrainingState(m) as flat:
        opt = FlatAdamW(flat, m, lr=1e-2, weight_decay=0.05)
        assert all(hasattr(layer.mixer.out_proj.weight, "_fv_shadow_pk2") for layer in m.layers)
        _assert_w2_current(m)
        before = m.layers[1].mixer.out_proj.weight._fv_shadow_pk2.clone()
        _train_step(m, flat, opt, x, tgt)
        _assert_w2_current(m)                                       # after an optimizer step
        assert not torch.equal(before, m.layers[1].mixer.out_proj.weight._fv_shadow_pk2)
        with torch.no_grad():                                       # after an in-place write: re-packed by the next use itself
            m.layers[1].mixer.out_proj.weight.add_(0.25)
        flat.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            (m(x).float() * tgt).sum().backward()
        flat.finish_backward()
        _assert_w2_current(m)
        sd = {k: (v * 0.75 if v.is_floating_point() else v) for k, v in m.state_dict().items()}
        m.load_state_dict(sd)                                       # after load_state_dict (post hook)
        _assert_w2_current(m)
    assert leftovers() == []                                        # gone after close() ...
    flat = FlatTrainingState(m)                                     # ... and, from a state that is never closed,
    assert leftovers() != []
    flat2 = FlatTrainingState(m, shadow_dtype=torch.float32)        # under a second state that keeps no bf16 copies
    assert leftovers() == []
    flat2.close()


def test_training_step_is_bit_identical_with_and_without_the_packed_w2(monkeypatch):
    from fastvim_amd import mamba_simple_faster as msf
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    base = _model()
    x = torch.randn(2, 3, 224, 224, device="cuda")
    tgt = torch.randn(2, 20, device="cuda")
    res = []
    for on in (True, False):
        m = copy.deepcopy(base)
        calls = {"pk2": 0}
        real_b = msf.M.conv_pool_bwd_dgrad
        monkeypatch.setattr(msf.M, "conv_pool_bwd_dgrad",
                            lambda *a, **k: (calls.__setitem__("pk2", calls["pk2"] + (k.get("W2_pk") is not None)), real_b(*a, **k))[1])
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
            monkeypatch.setattr(msf.M, "conv_pool_bwd_dgrad", real_b)
        if on:
            assert calls["pk2"] > 0, calls                          # the packed second phase was really taken
        else:
            assert calls["pk2"] == 0, calls
    for (l1, g1), (l0, g0) in zip(res[0][0], res[1][0]):
        assert torch.equal(l1, l0) and torch.equal(g1, g0)
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])


def test_graph_replay_equals_eager_with_the_packed_w2():
    import fastvim_amd
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    from fastvim_amd.pipeline import SegmentedTrainStep
    if not fastvim_amd.graph_capture_safe():
        pytest.skip("HIP graph capture is not safe in this process")
    base = _model(drop_path=0.0)
    x = torch.randn(2, 3, 224, 224, device="cuda")
    tgt = torch.randn(2, 20, device="cuda")
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
            _assert_w2_current(m)
            res.append((torch.stack(losses), flat.param_flat.clone(), flat.grad_flat.clone()))
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
