"""MAE pre-training from uint8 batches: with the normalisation table attached, ``MaskedAutoencoderViM`` takes the 8-bit
batch itself -- the patch embedding and the reconstruction loss look the pixels up inside their kernels -- and computes,
bit for bit, what it computes from the normalised float batch with ``fused_loss=True``.

The model is the small one tests/test_mae_gpu.py steps against the oracle (embed 192, depth 3, decoder 128 x 1, batch 2,
224 px, fixed masking noise); the huge factory (patch 14, 224 px: the 16 x 16 grid it is trained on) at depth 2 covers the
other patch size."""
import pytest
import torch

import mae_loss_ref as R
from test_mae_loss_gpu import bounds

pytestmark = pytest.mark.gpu
F64 = torch.float64


def _small(**kw):
    from fastvim_amd.models_mae import MaskedAutoencoderViM
    torch.manual_seed(3)
    return MaskedAutoencoderViM(img_size=224, patch_size=16, depth=3, embed_dim=192, decoder_embed_dim=128, decoder_depth=1,
                                rms_norm=True, residual_in_fp32=True, fused_add_norm=True, **kw).cuda()


def _huge(**kw):
    from fastvim_amd.models_mae import mae_FastVim_huge_dec512d2b
    torch.manual_seed(3)
    return mae_FastVim_huge_dec512d2b(img_size=224, depth=2, **kw).cuda()


def _attach(m):
    from fastvim_amd.pixels import IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD, attach_pixel_norm
    return attach_pixel_norm(m, IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD)


def _batch(px, L, seed=4, n=2):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (n, 3, px, px), generator=g, dtype=torch.uint8)
    noise = torch.rand(n, L, generator=torch.Generator().manual_seed(seed + 1))
    return x.cuda(), noise.cuda()


def _step(m, flat, x, noise, autocast):
    flat.zero_grad()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        loss, pred, mask = m(x, noise=noise)
    loss.backward()
    flat.finish_backward()
    return loss.detach().clone(), pred.detach().clone(), mask.clone(), flat.grad_flat.clone()


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("which", ["small16", "huge14"])
def test_uint8_batch_equals_the_float_batch_bit_for_bit(which, autocast):
    """Fails with ``TypeError`` before uint8 batches were supported."""
    from fastvim_amd.flat import FlatTrainingState
    m = (_small if which == "small16" else _huge)(fused_loss=True)
    pn = _attach(m)
    px, L = (224, 196) if which == "small16" else (224, 256)
    x, noise = _batch(px, L)
    flat = FlatTrainingState(m)
    try:
        a = _step(m, flat, x, noise, autocast)
        b = _step(m, flat, pn(x), noise, autocast)
    finally:
        flat.close()
    for name, u, v in zip(("loss", "pred", "mask", "grad_flat"), a, b):
        assert torch.equal(u, v), name
    assert torch.isfinite(a[0]).item() and a[3].abs().max().item() > 0


def test_uint8_loss_against_the_composition_and_the_oracle():
    """The loss from the uint8 batch (fused kernel) against the same model with the eager composition on the normalised
    batch, and against the fp64 oracle of the whole model: the kernel test's bound for (patch 16, fp32) on the loss
    itself; against the oracle the bound tests/test_mae_gpu.py holds the fp32 model to (the encoder / decoder error, which
    the loss kernel does not change)."""
    from oracle import mae_forward_oracle
    m = _small()
    pn = _attach(m)
    x, noise = _batch(224, 196)
    xf = pn(x)
    with torch.no_grad():
        lu, pu, mu = m(x, noise=noise)
        assert m.fused_loss is False
        le, pe, me = m(xf, noise=noise)
    assert torch.equal(pu, pe) and torch.equal(mu, me)
    ref = R.mae_loss_ref(xf.cpu(), pu.cpu(), mu.cpu(), 16, True)
    bl, _ = bounds(16, False)
    print(f"fused {lu.item()!r} eager {le.item()!r} fp64-of-same-pred {ref['loss'].item()!r}")
    assert abs(lu.item() - ref["loss"].item()) <= bl * abs(ref["loss"].item())
    assert abs(lu.item() - le.item()) <= bl * abs(ref["loss"].item())
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    lref, _, mref = mae_forward_oracle(sd, xf.cpu(), noise.cpu(), depth=3, decoder_depth=1, compute_dtype=F64)
    assert torch.equal(mu.cpu().double(), mref)
    assert abs(lu.item() - lref.item()) <= 5e-5 * max(1.0, abs(lref.item()))


def test_graph_replay_from_a_uint8_static_buffer_equals_eager_steps():
    """Forward + backward + optimizer step captured by hand over a uint8 static buffer that is refilled between replays:
    three replays equal three eager steps on the same batches, bit for bit."""
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    batches = [_batch(224, 196, seed=10 + 2 * i) for i in range(5)]

    def make():
        m = _small().train()
        _attach(m)
        flat = FlatTrainingState(m)
        opt = FlatAdamW(flat, m, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.05, ema_decay=0.9999)
        return m, flat, opt

    def one_step(m, flat, opt, x, noise):
        flat.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = m(x, noise=noise)[0]
        loss.backward()
        flat.finish_backward()
        opt.step()
        return loss.detach()

    m1, f1, o1 = make()
    try:
        eager = [one_step(m1, f1, o1, x, n).item() for x, n in batches]
        p_eager = f1.param_flat.clone()
    finally:
        f1.close()
    m2, f2, o2 = make()
    try:
        xs, ns = torch.empty_like(batches[0][0]), torch.empty_like(batches[0][1])
        assert xs.dtype == torch.uint8
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        got = []
        with torch.cuda.stream(side):
            for x, n in batches[:2]:
                xs.copy_(x)
                ns.copy_(n)
                got.append(one_step(m2, f2, o2, xs, ns).item())
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            lb = one_step(m2, f2, o2, xs, ns)
        for x, n in batches[2:]:
            xs.copy_(x)
            ns.copy_(n)
            graph.replay()
            got.append(lb.item())
        torch.cuda.synchronize()
        assert got == eager, (got, eager)
        assert torch.equal(f2.param_flat, p_eager)
    finally:
        f2.close()


def test_float_images_without_fused_loss_are_the_parents_forward():
    """``fused_loss=False`` (the default) with float images: ``forward`` returns ``forward_loss`` of its own pred and mask,
    the eager composition, bit for bit; switching the attribute on changes the loss only within the kernel's bound."""
    m = _small()
    x, noise = _batch(224, 196)
    xf = _attach(m)(x)
    with torch.no_grad():
        loss, pred, mask = m(xf, noise=noise)
        assert torch.equal(loss, m.forward_loss(xf, pred, mask))
        m.fused_loss = True
        lf, pf, mf = m(xf, noise=noise)
    assert torch.equal(pf, pred) and torch.equal(mf, mask)
    ref = R.mae_loss_ref(xf.cpu(), pred.cpu(), mask.cpu(), 16, True)
    assert abs(lf.item() - ref["loss"].item()) <= bounds(16, False)[0] * abs(ref["loss"].item())
