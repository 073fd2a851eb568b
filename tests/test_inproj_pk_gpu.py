"""in_proj forward with its weight streamed in MFMA fragment order (mixer_ops.pack_index_in, fv_gemm_bf16_inproj_pk): the batched
pack kernel against the gather the map defines, the launch BIT FOR BIT against gemm_nt (same MFMA, operand order and k order)
between guard rows, the callers that must keep the plain GEMM, and the flat training state's new shadow: kept current, used by
the training step without changing one bit of it, snapshotted by the segmented step and never left behind on a model."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

N, K = 768, 192
SENTINEL = 0x5A5B          # bf16 bit pattern C's guard rows (and C itself) are pre-filled with


def _random_bf16_bits(shape, seed):
    """Random bf16 BIT PATTERNS (NaNs, infinities and denormals included): a permutation copy must move them all."""
    g = torch.Generator().manual_seed(seed)
    bits = torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int32).to(torch.int16)
    return bits.cuda().view(torch.bfloat16)


def _same_bits(a, b):
    v = torch.int16 if a.element_size() == 2 else torch.int32
    return torch.equal(a.view(v), b.view(v))


@pytest.mark.parametrize("njobs", [1, 24])
def test_pack_in_kernel_equals_the_gather_of_pack_index_in(njobs):
    from fastvim_amd import mixer_ops as M
    srcs = [_random_bf16_bits((N, K), seed=100 * njobs + j) for j in range(njobs)]
    dsts = [torch.zeros(N * K, device="cuda", dtype=torch.bfloat16) for _ in range(njobs)]
    M.pack_weight_frags_in(srcs, dsts)
    torch.cuda.synchronize()
    for s, d_ in zip(srcs, dsts):
        ref = M.pack_weight_frags_in_ref(s.view(torch.int16))
        assert torch.equal(d_.view(torch.int16), ref.reshape(-1))


@pytest.fixture(scope="module")
def weight():
    from fastvim_amd import mixer_ops as M
    g = torch.Generator().manual_seed(11)
    W = (torch.randn(N, K, generator=g) * K ** -0.5).to("cuda", torch.bfloat16)
    W_pk = torch.empty(N * K, device="cuda", dtype=torch.bfloat16)
    M.pack_weight_frags_in([W], [W_pk])
    return W, W_pk


# single row, partial tile, exact tile, tile + 1, two images, three images; rows per workgroup: the library's choice, the
# 49 of the even deal at batch 128, the even deal itself (16 at these sizes: several tiles from M = 49 on)
@pytest.mark.parametrize("Mrows", [1, 49, 63, 64, 65, 392, 588])
@pytest.mark.parametrize("rows_per_tile", [0, 49, -1])
def test_launch_equals_gemm_nt_bit_for_bit(weight, Mrows, rows_per_tile):
    import ctypes
    from fastvim_amd import _lib as L_
    from fastvim_amd.gemm import gemm_nt
    W, W_pk = weight
    G = 64                                                                       # guard rows on either side
    g = torch.Generator().manual_seed(1000 + Mrows)
    a_all = torch.full((Mrows + G, K), float("nan"), device="cuda", dtype=torch.bfloat16)      # A, then NaN rows
    a_all[:Mrows] = torch.randn(Mrows, K, generator=g).to("cuda", torch.bfloat16)
    A = a_all[:Mrows]
    c_all = torch.full((Mrows + 2 * G, N), SENTINEL, device="cuda", dtype=torch.int16).view(torch.bfloat16)
    C = c_all[G:G + Mrows]
    rc = L_.lib().fv_gemm_bf16_inproj_pk(L_.ptr(A), L_.ptr(W_pk), L_.ptr(C), L_.i32(Mrows), L_.i32(N), L_.i32(K), ctypes.c_long(K),
                                         L_.i32(rows_per_tile), L_.stream_of(A))
    L_.check(rc, "gemm_bf16_inproj_pk")
    ref = gemm_nt(A, W)
    torch.cuda.synchronize()
    assert torch.isfinite(ref.float()).all()
    assert _same_bits(C, ref)
    bits = c_all.view(torch.int16)
    assert (bits[:G] == SENTINEL).all() and (bits[G + Mrows:] == SENTINEL).all()


def test_launch_refuses_what_it_was_not_built_for(weight):
    import ctypes
    from fastvim_amd import _lib as L_
    W, W_pk = weight
    A = torch.zeros(64, 2 * K, device="cuda", dtype=torch.bfloat16)
    C = torch.zeros(64, N, device="cuda", dtype=torch.bfloat16)
    call = lambda a, n, k, lda: L_.lib().fv_gemm_bf16_inproj_pk(L_.ptr(a), L_.ptr(W_pk), L_.ptr(C), L_.i32(64), L_.i32(n), L_.i32(k),
                                                                ctypes.c_long(lda), L_.i32(0), L_.stream_of(a))
    assert call(A, N, K, 2 * K) != 0                       # lda != K
    assert call(A, N, 2 * K, 2 * K) != 0                   # K != 192
    assert call(A, 640, K, K) != 0                         # N not a multiple of 384
    assert call(A.view(-1)[4:4 + 64 * K], N, K, K) != 0    # A not 16-byte aligned
    assert call(A, N, K, K) == 0
    torch.cuda.synchronize()


def test_ineligible_callers_take_the_plain_gemm_with_the_same_values(weight, monkeypatch):
    from fastvim_amd import mamba_simple_faster as msf
    from fastvim_amd.gemm import gemm_nt
    W, W_pk = weight
    Wp = torch.nn.Parameter(W.float())
    Wp._fv_shadow_pk_in = W_pk
    Wp._fv_shadow_pk_in_version = Wp._version
    calls = {"pk": 0}
    real = msf.M.in_proj_fwd_pk
    monkeypatch.setattr(msf.M, "in_proj_fwd_pk", lambda *a, **k: (calls.__setitem__("pk", calls["pk"] + 1), real(*a, **k))[1])
    g = torch.Generator().manual_seed(5)
    wide = torch.randn(130, 2 * K, generator=g).to("cuda", torch.bfloat16)
    A = wide[:, :K].contiguous()
    ref = gemm_nt(A, W)
    got = msf.in_proj_fwd(A, Wp, W, None, torch.bfloat16)                         # eligible: the packed launch
    assert calls["pk"] == 1 and _same_bits(got, ref)
    got = msf.in_proj_fwd(wide[:, :K], Wp, W, None, torch.bfloat16)               # lda != K: plain
    assert calls["pk"] == 1 and _same_bits(got, ref)
    bias = torch.randn(N, generator=g).cuda()
    got = msf.in_proj_fwd(A, Wp, W, bias, torch.bfloat16)                         # bias: plain
    assert calls["pk"] == 1 and _same_bits(got, gemm_nt(A, W, bias=bias))
    was = msf.use_packed_weights(False)                                           # switched off: plain
    try:
        got = msf.in_proj_fwd(A, Wp, W, None, torch.bfloat16)
    finally:
        msf.use_packed_weights(was)
    assert calls["pk"] == 1 and _same_bits(got, ref)
    got = msf.in_proj_fwd(A, torch.nn.Parameter(W.float()), W, None, torch.bfloat16)      # no flat state, no copy: plain
    assert calls["pk"] == 1 and _same_bits(got, ref)
    torch.cuda.synchronize()


def _model(depth=3, classes=20, drop_path=0.1):
    from fastvim_amd.fastvim import VisionMamba
    torch.manual_seed(0)
    return VisionMamba(img_size=224, depth=depth, embed_dim=192, num_classes=classes, rms_norm=True, residual_in_fp32=True,
                       fused_add_norm=True, final_pool_type="mean", if_abs_pos_embed=True, drop_path_rate=drop_path).cuda().train()


def _assert_in_current(m):
    """Every in_proj shadow is pack_index_in of the current bf16 shadow, and that shadow is the bf16 cast of the fp32 master."""
    from fastvim_amd.mixer_ops import pack_weight_frags_in_ref
    torch.cuda.synchronize()
    for layer in m.layers:
        w = layer.mixer.in_proj.weight
        sh = w._fv_shadow
        assert torch.equal(sh, w.detach().to(torch.bfloat16))
        assert torch.equal(w._fv_shadow_pk_in.view(torch.int16), pack_weight_frags_in_ref(sh.view(torch.int16)).reshape(-1))


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


def test_flat_state_keeps_the_in_proj_shadow_current_and_drops_it():
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    m = _model()
    x = torch.randn(2, 3, 224, 224, device="cuda")
    tgt = torch.randn(2, 20, device="cuda")
    attrs = ("_fv_shadow_pk_in", "_fv_shadow_pk_in_version")
    leftovers = lambda: [(n, a) for n, p in m.named_parameters() for a in attrs if hasattr(p, a)]
    with FlatTrainingState(m) as flat:
        opt = FlatAdamW(flat, m, lr=1e-2, weight_decay=0.05)
        assert all(hasattr(layer.mixer.in_proj.weight, "_fv_shadow_pk_in") for layer in m.layers)
        assert all(any(layer.mixer.in_proj.weight._fv_shadow_pk_in is b for b in flat._pk_dst) for layer in m.layers)
        _assert_in_current(m)
        before = m.layers[1].mixer.in_proj.weight._fv_shadow_pk_in.clone()
        _train_step(m, flat, opt, x, tgt)
        _assert_in_current(m)                                       # after an optimizer step
        assert not torch.equal(before, m.layers[1].mixer.in_proj.weight._fv_shadow_pk_in)
        with torch.no_grad():                                       # after an in-place write: re-packed by the next use itself
            m.layers[1].mixer.in_proj.weight.add_(0.25)
        flat.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            (m(x).float() * tgt).sum().backward()
        flat.finish_backward()
        _assert_in_current(m)
        sd = {k: (v * 0.75 if v.is_floating_point() else v) for k, v in m.state_dict().items()}
        m.load_state_dict(sd)                                       # after load_state_dict (post hook)
        _assert_in_current(m)
    assert leftovers() == []                                        # gone after close() ...
    flat = FlatTrainingState(m)                                     # ... and, from a state that is never closed,
    assert leftovers() != []
    flat2 = FlatTrainingState(m, shadow_dtype=torch.float32)        # under a second state that keeps no bf16 copies
    assert leftovers() == []
    flat2.close()


def test_segmented_step_snapshots_the_in_proj_shadow():
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    from fastvim_amd.pipeline import SegmentedTrainStep
    m = _model(drop_path=0.0)
    x = torch.randn(2, 3, 224, 224, device="cuda")
    tgt = torch.randn(2, 20, device="cuda")
    with FlatTrainingState(m) as flat:
        opt = FlatAdamW(flat, m, lr=1e-2, weight_decay=0.05)
        step = SegmentedTrainStep(m, flat, opt, lambda lg, t_: (lg.float() * t_).sum(), x, tgt, n_segments=1, use_graph=False)
        snap = step._snapshot()
        held = [b for b, _ in snap[0]]
        for layer in m.layers:
            pk = layer.mixer.in_proj.weight._fv_shadow_pk_in
            assert any(pk is b for b in held)
        # a step advances the copies; restoring the snapshot puts them back
        saved = m.layers[0].mixer.in_proj.weight._fv_shadow_pk_in.clone()
        step.step()
        torch.cuda.synchronize()
        assert not torch.equal(saved, m.layers[0].mixer.in_proj.weight._fv_shadow_pk_in)
        step._restore(snap)
        torch.cuda.synchronize()
        assert torch.equal(saved, m.layers[0].mixer.in_proj.weight._fv_shadow_pk_in)
        _assert_in_current(m)


def test_training_step_is_bit_identical_with_and_without_the_packed_in_proj(monkeypatch):
    from fastvim_amd import mamba_simple_faster as msf
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    base = _model()
    x = torch.randn(2, 3, 224, 224, device="cuda")
    tgt = torch.randn(2, 20, device="cuda")
    res = []
    for on in (True, False):
        m = copy.deepcopy(base)
        calls = {"pk": 0}
        real = msf.M.in_proj_fwd_pk
        monkeypatch.setattr(msf.M, "in_proj_fwd_pk", lambda *a, **k: (calls.__setitem__("pk", calls["pk"] + 1), real(*a, **k))[1])
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
            monkeypatch.setattr(msf.M, "in_proj_fwd_pk", real)
        assert calls["pk"] == (2 * 3 if on else 0), calls             # every block, the first one included -- or none
    for (l1, g1), (l0, g0) in zip(res[0][0], res[1][0]):
        assert torch.equal(l1, l0) and torch.equal(g1, g0)
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])


def test_graph_replay_equals_eager_with_the_packed_in_proj():
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
            _assert_in_current(m)
            res.append((torch.stack(losses), flat.param_flat.clone(), flat.grad_flat.clone()))
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
