"""``fastvim_amd.chan_tokens`` (csrc/chan_tokens.hip) against its restatement (tests/chan_cls_tokens_ref.py, which
tests/test_chan_cls_tokens_cpu.py holds to the torch chain of ``models_channel_mamba.VisionMamba.forward_features``): the
tokens and ``dy`` bit for bit, ``d cls_token`` within one fp32 rounding of the fp64 sum of the same terms; a captured call
replayed on new inputs; the op outside its predicate."""
import pytest
import torch

import chan_cls_tokens_ref as R
from mae_tokens_cls_ref import sum_bound

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
BATCHES, LENS = (1, 3), (1, 2, 7, 12)            # the smallest sequence, odd M, M = P C' with P = 4
DIMS = (4, 8, 36, 384)                           # one unit a row; one 8-wide unit; % 4 but not % 8 (bf16: 4-wide units); ChannelVim-S


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _inputs(B, M, D, dtype, seed):
    g = torch.Generator().manual_seed(seed + B * 1000 + M * 50 + D)
    y = torch.randn(B, M, D, generator=g).to(dtype)
    y.view(-1)[0] = -0.0
    cls = 0.02 * torch.randn(1, 1, D, generator=g)
    dout = torch.randn(B, M + 1, D, generator=g).to(dtype)
    dout.view(-1)[-1] = -0.0
    return y.cuda(), cls.cuda(), dout.cuda()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("D", DIMS)
def test_kernels_equal_the_restatement(D, dtype):
    from fastvim_amd import chan_tokens as T
    worst = 0.0
    for B in BATCHES:
        for M in LENS:
            for p in sorted({0, M // 2, M}):
                y, cls, dout = _inputs(B, M, D, dtype, p)
                want, (want_dy, terms) = R.fwd(y, cls, p), R.bwd(dout, p)
                runs = []
                for _ in range(2):
                    ya, ca = y.clone().requires_grad_(True), cls.clone().requires_grad_(True)
                    assert T.chan_cls_tokens_ok(ya, ca, p)
                    out = T.chan_cls_tokens(ya, ca, p)
                    out.backward(dout)
                    runs.append((out.detach(), ya.grad, ca.grad))
                out, dy, dcls = runs[0]
                where = (B, M, D, p)
                assert out.dtype == dtype and out.shape == (B, M + 1, D) and torch.equal(_bits(out), _bits(want)), where
                assert dy.dtype == dtype and dy.shape == (B, M, D) and torch.equal(_bits(dy), _bits(want_dy)), where
                assert dcls.dtype == torch.float32 and dcls.shape == cls.shape, where
                err = (dcls.double().view(-1) - terms.sum(0)).abs()
                bound = sum_bound(terms)
                worst = max(worst, (err / bound.clamp_min(1e-300)).max().item())
                assert bool((err <= bound).all()), where
                assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(runs[0], runs[1])), where      # the same bits again
    print(f"d cls_token: max err/bound {worst:.3f}")


def test_more_than_one_workgroup_and_the_model_shape():
    """ChannelVim-S/16 at one sample and 3 channels (588 tokens, D 384): many workgroups each way, class row in the middle."""
    from fastvim_amd import chan_tokens as T
    B, M, D, p = 3, 588, 384, 294
    for dtype in DTYPES:
        y, cls, dout = _inputs(B, M, D, dtype, 9)
        ya, ca = y.clone().requires_grad_(True), cls.clone().requires_grad_(True)
        out = T.assemble(ya, ca, p)
        out.backward(dout)
        want_dy, terms = R.bwd(dout, p)
        assert torch.equal(_bits(out), _bits(R.fwd(y, cls, p))) and torch.equal(_bits(ya.grad), _bits(want_dy))
        assert bool(((ca.grad.double().view(-1) - terms.sum(0)).abs() <= sum_bound(terms)).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_captured_call_replays_on_new_inputs(dtype):
    from fastvim_amd import chan_tokens as T
    B, M, D, p = 3, 12, 36, 6
    y, cls, dout = _inputs(B, M, D, dtype, 1)
    ys, cs, ds = y.clone().requires_grad_(True), cls.clone().requires_grad_(True), dout.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                             # warm-up outside the capture
        T.chan_cls_tokens(ys, cs, p).backward(ds)
    torch.cuda.current_stream().wait_stream(side)
    ys.grad = cs.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = T.chan_cls_tokens(ys, cs, p)
        gy, gc = torch.autograd.grad(out, (ys, cs), ds)
    for seed in (2, 3):
        y2, cls2, dout2 = _inputs(B, M, D, dtype, seed)
        with torch.no_grad():
            ys.copy_(y2)
            cs.copy_(cls2)
            ds.copy_(dout2)
        graph.replay()
        torch.cuda.synchronize()
        want_dy, terms = R.bwd(dout2, p)
        assert torch.equal(_bits(out), _bits(R.fwd(y2, cls2, p))) and torch.equal(_bits(gy), _bits(want_dy))
        assert bool(((gc.double().view(-1) - terms.sum(0)).abs() <= sum_bound(terms)).all())
    assert not torch.equal(out, R.fwd(y, cls, p))             # (the inputs did change)


@pytest.mark.parametrize("what", ["cpu", "non_contiguous", "D=30", "fp16", "p=M+1"])
def test_op_raises_outside_its_predicate_and_the_chooser_takes_the_chain(what):
    from fastvim_amd import chan_tokens as T
    g = torch.Generator().manual_seed(3)
    B, M, D, p = 2, 12, (30 if what == "D=30" else 32), (13 if what == "p=M+1" else 6)
    dev = "cpu" if what == "cpu" else "cuda"
    y = torch.randn(B, M, D, generator=g).to(dev)
    if what == "non_contiguous":
        y = torch.randn(B, D, M, generator=g).to(dev).transpose(1, 2)
    if what == "fp16":
        y = y.half()
    cls = torch.randn(1, 1, D, generator=g).to(dev)
    assert not T.chan_cls_tokens_ok(y, cls, p)
    with pytest.raises(RuntimeError, match="chan_cls_tokens_ok"):
        T.chan_cls_tokens(y, cls, p)
    if what == "p=M+1":
        return
    ya, ca = y.clone().requires_grad_(True), cls.clone().requires_grad_(True)
    if what == "non_contiguous":
        ya = y.detach().requires_grad_(True)
    out = T.assemble(ya, ca, p)
    assert torch.equal(out, R.fwd(y, cls, p))
    dout = torch.randn(B, M + 1, D, generator=g).to(dev).to(y.dtype)
    out.backward(dout)
    dy, terms = R.bwd(dout, p)
    assert torch.equal(ya.grad, dy)
    ulp = 2.0 ** -24 * B                                      # autograd adds the B terms in fp32, in an order of its own
    assert bool(((ca.grad.double().view(-1) - terms.sum(0)).abs() <= ulp * terms.abs().sum(0)).all())


def test_entry_points_check_their_arguments():
    """The C entry points refuse what the predicate refuses (no launch is made): a dimension that is no multiple of 4, a
    class position outside 0 .. M, an unknown dtype."""
    from fastvim_amd import _lib as L
    y, cls, out = torch.zeros(2, 12, 32, device="cuda"), torch.zeros(32, device="cuda"), torch.zeros(2, 13, 32, device="cuda")
    lib = L.lib()

    def call(dtype, M, D, p):
        return lib.fv_chan_cls_tokens_fwd(L.ptr(y), L.i32(dtype), L.ptr(cls), L.ptr(out), L.i32(2), L.i32(M), L.i32(D), L.i32(p),
                                          L.stream_of(y))
    assert call(L.FV_F32, 12, 32, 6) == 0
    assert call(L.FV_F32, 12, 30, 6) != 0 and b"multiple of 4" in lib.fv_last_error()
    assert call(L.FV_F32, 12, 32, 13) != 0 and call(L.FV_F32, 12, 32, -1) != 0
    assert call(L.FV_F16, 12, 32, 6) != 0
    rc = lib.fv_chan_cls_tokens_bwd(L.ptr(out), L.ptr(y), L.i32(L.FV_F32), L.ptr(cls), L.i32(2), L.i32(12), L.i32(32), L.i32(13),
                                    L.stream_of(y))
    assert rc != 0
    torch.cuda.synchronize()
