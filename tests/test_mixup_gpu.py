"""Batch-mode Mixup / CutMix and the label losses on the GPU (csrc/glue.hip: fv_mix_batch, fv_patch_unfold_mix;
csrc/loss.hip: fv_mixup_target, fv_label_ce).

Bit-exact checks are against torch's own expressions on the same device (what timm.data.Mixup runs: ``x.mul(lam).add_(
x.flip(0).mul_(1. - lam))``, slice assignment from ``x.flip(0)``, ``one_hot * lam + one_hot.flip(0) * (1. - lam)``) and
against this package's dense kernels; the plain label losses are checked against the fp64 oracle; the graph-replayed
training step with mixup on is checked, bit for bit, against the same step fed torch-mixed images and dense targets."""
import copy

import numpy as np
import pytest
import torch

from fastvim_amd.mixup import Mixup

pytestmark = pytest.mark.gpu

# (lam, use_cutmix, box) per case, for an H x W image: mixup, cutmix with an interior box, a box clipped at two edges,
# an empty box, and lam = 1
def _cases(H, W):
    return [("mixup", 0.3172, False, None),
            ("mixup_small", 0.0431, False, None),
            ("cutmix_interior", 0.8, True, (H // 4, H // 2 + 1, W // 4 + 1, W // 2 + 3)),
            ("cutmix_clipped", 0.6, True, (0, H // 3, W - W // 3 - 1, W)),
            ("cutmix_empty", 1.0, True, (H // 2, H // 2, W // 2, W // 2 + 2)),
            ("lam_one", 1.0, False, None)]


def torch_mix(x, lam, use_cutmix, box):
    """timm.data.Mixup._mix_batch on a clone (timm works in place): returns the mixed batch."""
    x = x.clone()
    if lam == 1. and not use_cutmix:
        return x
    if use_cutmix:
        yl, yh, xl, xh = box
        x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
    else:
        x_flipped = x.flip(0).mul_(1. - lam)
        x.mul_(lam).add_(x_flipped)
    return x


def torch_target(labels, num_classes, lam, smoothing):
    """timm.data.mixup.mixup_target / one_hot."""
    off = smoothing / num_classes
    on = 1. - smoothing + off

    def one_hot(y):
        return torch.full((y.shape[0], num_classes), off, device=y.device).scatter_(1, y.view(-1, 1), on)
    return one_hot(labels) * lam + one_hot(labels.flip(0)) * (1. - lam)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(128, 3, 224, 224), (8, 3, 64, 48), (2, 1, 16, 16), (4, 2, 7, 9)])
def test_mix_batch_bitwise(shape, dtype):
    torch.manual_seed(sum(shape))
    x = torch.randn(shape, device="cuda").to(dtype)
    x0 = x.clone()
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0)
    for name, lam, cut, box in _cases(shape[2], shape[3]):
        mix.set(lam, use_cutmix=cut, box=box)
        got = mix.mix_batch(x)
        ref = torch_mix(x, lam, cut, box)
        assert got.dtype == dtype and got.data_ptr() != x.data_ptr()
        assert torch.equal(got, ref), (name, (got.float() - ref.float()).abs().max().item(), (got != ref).float().mean().item())
        assert torch.equal(x, x0)                                   # out of place: the input is untouched
        if name.startswith("mixup"):
            assert not torch.equal(got, x)
        if name == "cutmix_interior":
            assert not torch.equal(got, x)
        if name in ("cutmix_empty", "lam_one"):
            assert torch.equal(got, x)


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape,patch", [((128, 3, 224, 224), 16), ((8, 3, 224, 224), 14), ((6, 3, 64, 64), 8), ((4, 3, 32, 48), 16),
                                         ((4, 1, 448, 448), 16)])
def test_patch_unfold_mix_bitwise(shape, patch, out_dtype):
    """fv_patch_unfold_mix(x) == fv_patch_unfold(torch-mixed x), bit for bit.  Patch 14 is not a multiple of 8: the unfold
    kernels do not apply there, and PatchEmbed takes fv_mix_batch + the strided copy -- checked through the module below."""
    from fastvim_amd import glue_ops as G
    torch.manual_seed(patch)
    x = torch.randn(shape, device="cuda")
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0)
    if not G.patch_unfold_ok(x, patch, patch):
        assert patch == 14
        with pytest.raises(RuntimeError, match="multiple of 8"):
            G.patch_unfold_mix(x, patch, patch, out_dtype, mix.block(x.device))
        return
    for name, lam, cut, box in _cases(shape[2], shape[3]):
        mix.set(lam, use_cutmix=cut, box=box)
        got = G.patch_unfold_mix(x, patch, patch, out_dtype, mix.block(x.device))
        ref = G.patch_unfold(torch_mix(x, lam, cut, box), patch, patch, out_dtype)
        assert got.dtype == out_dtype and got.shape == ref.shape
        assert torch.equal(got, ref), (name, (got.float() - ref.float()).abs().max().item())
        # and the stand-alone op composes to the same bits (also for bf16 images: mixed in bf16, as torch mixes them)
        assert torch.equal(G.patch_unfold(mix.mix_batch(x), patch, patch, out_dtype), ref)
    xb = x[:8].to(torch.bfloat16).contiguous()
    mix.set(0.3172)
    assert torch.equal(G.patch_unfold_mix(xb, patch, patch, out_dtype, mix.block(x.device)),
                       G.patch_unfold(torch_mix(xb, 0.3172, False, None), patch, patch, out_dtype))


@pytest.mark.parametrize("patch", [16, 14, 8])
def test_patch_embed_with_mix(patch):
    """PatchEmbed.forward(x, mix=) == PatchEmbed.forward(torch-mixed x): through the fused unfold (16, 8) and through the
    fv_mix_batch fallback (14, where the unfold kernel does not apply)."""
    from fastvim_amd.fastvim import PatchEmbed
    torch.manual_seed(patch)
    size = patch * 6
    pe = PatchEmbed(img_size=size, patch_size=patch, in_chans=3, embed_dim=192).cuda()
    x = torch.randn(6, 3, size, size, device="cuda")
    pos = torch.randn(1, 36, 192, device="cuda")
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0)
    for name, lam, cut, box in _cases(size, size):
        mix.set(lam, use_cutmix=cut, box=box)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            got = pe(x, pos_embed=pos, mix=mix)
            ref = pe(torch_mix(x, lam, cut, box), pos_embed=pos)
        assert torch.equal(got, ref), name


@pytest.mark.parametrize("B,C,smoothing", [(128, 1000, 0.1), (6, 10, 0.1), (4, 2048, 0.0), (8, 3, 0.25)])
def test_mixup_target_bitwise(B, C, smoothing):
    torch.manual_seed(B)
    labels = torch.randint(0, C, (B,), device="cuda")
    labels[B - 1] = labels[0]                                       # a pair with equal labels
    labels[B - 2] = (labels[1] + 1) % C
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=smoothing, num_classes=C)
    for lam in (0.3172, 0.0431, 1.0, 0.0, 0.9999999):
        mix.set(lam)
        got = mix.target(labels)
        ref = torch_target(labels, C, lam, smoothing)
        assert got.dtype == torch.float32 and torch.equal(got, ref), (lam, (got - ref).abs().max().item())


def test_call_is_the_drop_in():
    """``x_mixed, target = mix(x, labels)``: draws like timm (numpy stream), mixes out of place, returns the dense target."""
    B, C = 8, 10
    torch.manual_seed(0)
    x = torch.randn(B, 3, 32, 48, device="cuda")
    labels = torch.randint(0, C, (B,), device="cuda")
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=C)
    np.random.seed(5)
    seen = set()
    for _ in range(12):
        gpu_rng = torch.cuda.get_rng_state()
        xm, t = mix(x, labels)
        assert torch.equal(torch.cuda.get_rng_state(), gpu_rng)
        p = mix.last()
        seen.add(p.use_cutmix)
        assert torch.equal(xm, torch_mix(x, p.lam, p.use_cutmix, p.box))
        assert torch.equal(t, torch_target(labels, C, p.lam, 0.1))
    assert seen == {True, False}
    np.random.seed(5)
    ref = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=C)
    ref.sample(x.shape)
    np.random.seed(5)
    mix(x, labels)
    assert mix.last() == ref.last()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,C", [(128, 1000), (6, 10), (4, 2048)])
def test_criterion_equals_dense_loss_bitwise(B, C, dtype):
    """mix.criterion()(x, labels) == SoftTargetCrossEntropy()(x, fv_mixup_target(labels)): loss and x.grad bit for bit, with
    a non-unit upstream scale; a repeat call is identical."""
    from fastvim_amd.losses import SoftTargetCrossEntropy
    torch.manual_seed(B + C)
    labels = torch.randint(0, C, (B,), device="cuda")
    labels[B - 1] = labels[0]
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=C)
    crit = mix.criterion()
    for lam in (0.3172, 1.0, 0.0431):
        mix.set(lam)
        x = (torch.randn(B, C, device="cuda") * 3).to(dtype).requires_grad_(True)
        loss = crit(x, labels)
        (loss * 2.5).backward()
        g = x.grad.clone()
        x.grad = None
        ref = SoftTargetCrossEntropy()(x, mix.target(labels))
        (ref * 2.5).backward()
        assert loss.dtype == torch.float32 and loss.dim() == 0 and g.dtype == dtype
        assert torch.equal(loss, ref) and torch.equal(g, x.grad), (lam, loss.item(), ref.item())
        assert torch.isfinite(loss).item() and g.abs().max().item() > 0
        x.grad = None
        loss2 = crit(x, labels)
        (loss2 * 2.5).backward()
        assert torch.equal(loss, loss2) and torch.equal(g, x.grad)


@pytest.mark.parametrize("B,C,dtype", [(128, 1000, torch.bfloat16), (128, 1000, torch.float32), (5, 10, torch.float32),
                                       (3, 2048, torch.bfloat16)])
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
def test_label_losses_vs_oracle(B, C, dtype, smoothing):
    """CrossEntropyLoss / LabelSmoothingCrossEntropy against the fp64 oracle on the dense target built here in fp64
    (confidence * one_hot + smoothing / C); the tolerances of test_soft_target_cross_entropy_vs_oracle."""
    from fastvim_amd.losses import CrossEntropyLoss, LabelSmoothingCrossEntropy
    from oracle import soft_target_ce_oracle
    torch.manual_seed(B + C)
    x = (torch.randn(B, C, device="cuda") * 3).to(dtype).requires_grad_(True)
    labels = torch.randint(0, C, (B,), device="cuda")
    t = torch.full((B, C), smoothing / C, dtype=torch.float64)
    t[torch.arange(B), labels.cpu()] += 1.0 - smoothing
    ref, gref = soft_target_ce_oracle(x, t)
    crit = CrossEntropyLoss() if smoothing == 0.0 else LabelSmoothingCrossEntropy(smoothing)
    loss = crit(x, labels)
    (loss * 2.5).backward()
    assert loss.dtype == torch.float32 and loss.dim() == 0
    print(f"loss {loss.item()} ref {ref.item()} grad err {(x.grad.double().cpu() - 2.5 * gref).abs().max().item()}")
    assert abs(loss.item() - ref.item()) <= 2e-5 * max(1.0, abs(ref.item()))
    tol = (1e-6 if dtype == torch.float32 else 2e-2) * gref.abs().max().item() * 2.5
    assert (x.grad.double().cpu() - 2.5 * gref).abs().max().item() <= tol
    if smoothing == 0.0 and dtype == torch.float32:
        tref = torch.nn.functional.cross_entropy(x.detach(), labels)
        assert abs(loss.item() - tref.item()) <= 2e-5 * max(1.0, abs(tref.item()))
    # validation: the same value, no gradient, plus the top-1 count
    val, n = crit.loss_and_correct(x.detach(), labels)
    assert torch.equal(val, loss.detach()) and n.dtype == torch.int32


@pytest.mark.parametrize("B,C,dtype", [(128, 1000, torch.bfloat16), (128, 1000, torch.float32), (7, 10, torch.float32),
                                       (5, 2048, torch.bfloat16)])
def test_top1_exact(B, C, dtype):
    """Random bf16 logits tie for the row maximum in a few percent of 1000-class rows, so the maximum is made unique: one
    chosen class per row is set to rowmax + 1, the label itself in about half the rows.  Every flag and the count exact."""
    from fastvim_amd.losses import CrossEntropyLoss, top1_correct
    torch.manual_seed(C)
    x = (torch.randn(B, C, device="cuda") * 3).to(dtype)
    labels = torch.randint(0, C, (B,), device="cuda")
    chosen = torch.where(torch.rand(B, device="cuda") < 0.5, labels, torch.randint(0, C, (B,), device="cuda"))
    x[torch.arange(B), chosen] = (x.float().max(dim=1).values + 1).to(dtype)
    want = chosen == labels
    assert 0 < want.sum().item() < B
    assert torch.equal(x.float().argmax(1), chosen)                 # the maximum is unique
    flags = top1_correct(x, labels)
    assert flags.dtype == torch.bool and torch.equal(flags, want)
    _, n = CrossEntropyLoss().loss_and_correct(x, labels)
    assert n.item() == want.sum().item()


class _NoMixKeyword(torch.nn.Module):
    """A model whose ``_embed`` has no ``mix`` keyword (the channel models, third-party backbones): SegmentedTrainStep mixes
    such a model's batch with one fv_mix_batch launch into a buffer of its own."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def _embed(self, x):
        return self.inner._embed(x)

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            return getattr(super().__getattr__("inner"), name)


@pytest.mark.parametrize("fallback", [False, True])
def test_graph_step_with_mixup_equals_step_on_torch_mixed_batches(fallback):
    """Graph replay on, bf16, a forced sequence of parameter sets (mixup, cutmix, lam = 1, mixup, cutmix), one per step:
    SegmentedTrainStep(..., mix.criterion(), x, labels, mixup=mix) leaves parameters, Adam moments, EMA and losses
    bit-identical to a second SegmentedTrainStep fed the torch-mixed images and the dense target through
    SoftTargetCrossEntropy -- the captured graphs pick up new values without recapture, and the fused unfold (or, with
    ``fallback``, the fv_mix_batch launch in front of a model without the keyword) changes nothing downstream."""
    from fastvim_amd.fastvim import VisionMamba
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    from fastvim_amd.losses import SoftTargetCrossEntropy
    from fastvim_amd.pipeline import SegmentedTrainStep
    B, C = 16, 100

    def make():
        torch.manual_seed(0)
        m = VisionMamba(img_size=224, depth=6, embed_dim=192, num_classes=C, rms_norm=True, residual_in_fp32=True,
                        fused_add_norm=True, final_pool_type="mean", if_abs_pos_embed=True, drop_path_rate=0.1).cuda().train()
        flat = FlatTrainingState(m)
        nd = {n for n, p in m.named_parameters() if p.ndim <= 1 or n.endswith(".bias") or n in m.no_weight_decay()
              or getattr(p, "_no_weight_decay", False)}
        return m, flat, FlatAdamW(flat, m, lr=1e-3, weight_decay=0.05, no_decay=nd, ema_decay=0.999)

    g = torch.Generator(device="cuda").manual_seed(11)
    batches = [(torch.randn(B, 3, 224, 224, device="cuda", generator=g), torch.randint(0, C, (B,), device="cuda", generator=g))
               for _ in range(2)]
    seq = [(0.3172, False, None), (0.71, True, (40, 150, 0, 97)), (1.0, False, None), (0.0431, False, None),
           (0.55, True, (200, 224, 100, 224))]

    # reference: torch-mixed images, dense targets
    m1, f1, o1 = make()
    x1 = torch.zeros(B, 3, 224, 224, device="cuda")
    t1 = torch.zeros(B, C, device="cuda")
    torch.manual_seed(7)
    ref_step = SegmentedTrainStep(m1, f1, o1, SoftTargetCrossEntropy(), x1, t1, n_segments=3, use_graph=True, warmup=2)
    assert ref_step.use_graph
    ref = []
    for i, (lam, cut, box) in enumerate(seq):
        xb, yb = batches[i % 2]
        x1.copy_(torch_mix(xb, lam, cut, box))
        t1.copy_(torch_target(yb, C, lam, 0.1))
        ref.append(ref_step.step().item())
    torch.cuda.synchronize()

    # under test: raw images, integer labels, the parameters through the device block
    m2, f2, o2 = make()
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=C)
    mix.set(0.5)                                                    # what the capture sees: none of the replayed values
    x2 = torch.zeros(B, 3, 224, 224, device="cuda")
    y2 = torch.zeros(B, dtype=torch.int64, device="cuda")
    model = _NoMixKeyword(m2) if fallback else m2
    torch.manual_seed(7)
    step = SegmentedTrainStep(model, f2, o2, mix.criterion(), x2, y2, n_segments=3, use_graph=True, warmup=2, mixup=mix)
    assert step.use_graph and step._embed_takes_mix is (not fallback) and (step._x_mixed is not None) is fallback
    got = []
    for i, (lam, cut, box) in enumerate(seq):
        xb, yb = batches[i % 2]
        x2.copy_(xb)
        y2.copy_(yb)
        mix.set(lam, use_cutmix=cut, box=box)
        got.append(step.step().item())
    torch.cuda.synchronize()
    assert torch.equal(x2, batches[(len(seq) - 1) % 2][0])         # the input buffer is never written by the step
    assert got == ref, (got, ref)
    assert len(set(got)) == len(got) and all(v == v for v in got)
    assert o2.step_t.item() == float(len(seq))
    assert torch.equal(f1.param_flat, f2.param_flat)
    assert torch.equal(o1.exp_avg, o2.exp_avg) and torch.equal(o1.exp_avg_sq, o2.exp_avg_sq)
    assert torch.equal(o1.ema, o2.ema)
    f1.close(); f2.close()


def test_eval_never_mixes():
    from fastvim_amd.fastvim import VisionMamba
    torch.manual_seed(0)
    m = VisionMamba(img_size=64, depth=2, embed_dim=192, num_classes=10, rms_norm=True, residual_in_fp32=True,
                    fused_add_norm=True, final_pool_type="mean", if_abs_pos_embed=True).cuda().eval()
    x = torch.randn(4, 3, 64, 64, device="cuda")
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, num_classes=10)
    mix.set(0.25)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        a, _ = m._embed(x, mix=mix)
        b, _ = m._embed(x)
        m.train()
        c, _ = m._embed(x, mix=mix)
    assert torch.equal(a, b) and not torch.equal(a, c)
