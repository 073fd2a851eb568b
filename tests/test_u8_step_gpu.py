"""uint8 input buffers through the modules and the graph-replayed step objects (fastvim_amd/pixels.py): everything equals a
twin fed ``PixelNorm(batch)`` -- the fp32 pixels a host-side loader would have produced -- bit for bit."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MEAN3, STD3 = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
MEAN8 = (0.0913, 0.1377, 0.2048, 0.0562, 0.3301, 0.4419, 0.0271, 0.1802)
STD8 = (0.0721, 0.1139, 0.1618, 0.0333, 0.2504, 0.2987, 0.0119, 0.0906)
B, CLASSES = 8, 10


def _fastvim(depth=3):
    from fastvim_amd.fastvim import VisionMamba
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    from fastvim_amd.pixels import attach_pixel_norm
    torch.manual_seed(0)
    m = VisionMamba(img_size=224, depth=depth, embed_dim=192, num_classes=CLASSES, rms_norm=True, residual_in_fp32=True,
                    fused_add_norm=True, final_pool_type="mean", if_abs_pos_embed=True, drop_path_rate=0.1).cuda().train()
    pn = attach_pixel_norm(m, MEAN3, STD3)
    flat = FlatTrainingState(m)
    nd = {n for n, p in m.named_parameters() if p.ndim <= 1 or n.endswith(".bias") or n in m.no_weight_decay()
          or getattr(p, "_no_weight_decay", False)}
    return m, flat, FlatAdamW(flat, m, lr=1e-3, weight_decay=0.05, no_decay=nd, ema_decay=0.999), pn


def _channel(depth=3):
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    from fastvim_amd.models_channel_mamba_faster import VisionMamba
    from fastvim_amd.pixels import attach_pixel_norm
    torch.manual_seed(0)
    m = VisionMamba(img_size=64, patch_size=16, depth=depth, embed_dim=192, channels=8, num_classes=CLASSES, rms_norm=True,
                    residual_in_fp32=True, fused_add_norm=True, final_pool_type="mean", if_abs_pos_embed=True,
                    drop_path_rate=0.1, hcs=True).cuda().train()
    pn = attach_pixel_norm(m, MEAN8, STD8)
    flat = FlatTrainingState(m)
    nd = {n for n, p in m.named_parameters() if p.ndim <= 1 or n.endswith(".bias") or n in m.no_weight_decay()
          or getattr(p, "_no_weight_decay", False)}
    return m, flat, FlatAdamW(flat, m, lr=1e-3, weight_decay=0.05, no_decay=nd, ema_decay=0.999), pn


def _batches(C, S, n=3, batch=B):
    g = torch.Generator(device="cuda").manual_seed(11)
    return [(torch.randint(0, 256, (batch, C, S, S), device="cuda", generator=g, dtype=torch.uint8),
             torch.randint(0, CLASSES, (batch,), device="cuda", generator=g)) for _ in range(n)]


@pytest.mark.parametrize("amp", [torch.bfloat16, torch.float32])
def test_eager_logits_from_uint8_equal_logits_from_normalised(amp):
    for make, C, S in ((_fastvim, 3, 224), (_channel, 8, 64)):
        m, flat, _, pn = make(depth=2)
        m.eval()
        x, _ = _batches(C, S, n=1, batch=4)[0]
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp == torch.bfloat16):
            got, want = m(x), m(pn(x))
        assert got.dtype == want.dtype and torch.equal(got, want)
        assert torch.isfinite(got).all()
        flat.close()


def test_graph_step_with_mixup_reads_the_new_bytes_every_replay():
    """SegmentedTrainStep, graph replay, Mixup on: three steps, a different uint8 batch copied into ``x`` before each; a twin
    is fed the fp32 normalised batches.  Loss and parameters bit-identical after every step."""
    from fastvim_amd.mixup import Mixup
    from fastvim_amd.pipeline import SegmentedTrainStep
    batches = _batches(3, 224)

    def run(u8):
        m, flat, opt, pn = _fastvim()
        mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=CLASSES)
        mix.set(0.5)
        x = torch.zeros(B, 3, 224, 224, device="cuda", dtype=torch.uint8 if u8 else torch.float32)
        y = torch.zeros(B, dtype=torch.int64, device="cuda")
        torch.manual_seed(7)
        step = SegmentedTrainStep(m, flat, opt, mix.criterion(), x, y, n_segments=3, use_graph=True, warmup=2, mixup=mix)
        assert step.use_graph and step._embed_takes_mix
        np.random.seed(3)
        rec = []
        for xb, yb in batches:
            x.copy_(xb if u8 else pn(xb))
            y.copy_(yb)
            mix.sample()
            loss = step.step().item()
            rec.append((loss, mix.last(), flat.param_flat.clone()))
        torch.cuda.synchronize()
        flat.close()
        return rec

    got, want = run(True), run(False)
    for (lg, pg, fg), (lw, pw_, fw) in zip(got, want):
        assert pg == pw_ and lg == lw and lg == lg, (lg, lw)
        assert torch.equal(fg, fw)
    assert len({l for l, _, _ in got}) == len(got)                 # three different batches gave three different losses


def test_graph_step_of_the_channel_model_with_a_sampler():
    """The channel model: subsets from a ChannelSampler, the table row looked up by the SOURCE channel inside the replay."""
    from fastvim_amd.hcs import ChannelSampler
    from fastvim_amd.pipeline import SegmentedTrainStep
    batches = _batches(8, 64)
    loss_fn = torch.nn.CrossEntropyLoss()

    def run(u8):
        m, flat, opt, pn = _channel()
        sampler = ChannelSampler(8)
        sampler.set([2, 5, 7])
        x = torch.zeros(B, 8, 64, 64, device="cuda", dtype=torch.uint8 if u8 else torch.float32)
        y = torch.zeros(B, dtype=torch.int64, device="cuda")
        torch.manual_seed(7)
        step = SegmentedTrainStep(m, flat, opt, loss_fn, x, y, n_segments=3, use_graph=True, warmup=2, hcs=sampler)
        assert step.use_graph
        random.seed(2)
        rec = []
        for xb, yb in batches:
            x.copy_(xb if u8 else pn(xb))
            y.copy_(yb)
            sampler.sample()
            rec.append((step.step().item(), list(sampler.last()), flat.param_flat.clone()))
        torch.cuda.synchronize()
        flat.close()
        return rec

    got, want = run(True), run(False)
    for (lg, sg, fg), (lw, sw, fw) in zip(got, want):
        assert sg == sw and lg == lw and lg == lg, (lg, lw)
        assert torch.equal(fg, fw)


def test_channel_model_step_with_mixup_mixes_after_normalising():
    """A model whose ``_embed`` takes no ``mix=``: the uint8 batch is normalised by the eager lookup and mixed after it, into a
    float ``_x_mixed`` -- one step equals the twin's."""
    from fastvim_amd.mixup import Mixup
    from fastvim_amd.pipeline import SegmentedTrainStep
    xb, yb = _batches(8, 64, n=1)[0]

    def run(u8):
        m, flat, opt, pn = _channel()
        m.patch_embed.hcs = False
        mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=CLASSES)
        mix.set(0.37)
        x = (xb if u8 else pn(xb)).clone()
        y = yb.clone()
        torch.manual_seed(7)
        step = SegmentedTrainStep(m, flat, opt, mix.criterion(), x, y, n_segments=3, use_graph=True, warmup=1, mixup=mix)
        assert step._x_mixed is not None and step._x_mixed.dtype == torch.float32 and not step._embed_takes_mix
        loss = step.step().item()
        out = (loss, flat.param_flat.clone(), step._x_mixed.clone())
        torch.cuda.synchronize()
        flat.close()
        return out

    got, want = run(True), run(False)
    assert got[0] == want[0] and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])


def test_validation_step_with_a_uint8_buffer_and_a_short_last_batch():
    from fastvim_amd.evaluate import ValidationStep
    m, flat, opt, pn = _fastvim()
    batches = _batches(3, 224, n=2, batch=4)
    xu = torch.zeros(4, 3, 224, 224, device="cuda", dtype=torch.uint8)
    xf = torch.zeros(4, 3, 224, 224, device="cuda")
    yv = torch.zeros(4, dtype=torch.int64, device="cuda")
    vu = ValidationStep(m, flat, opt, xu, yv)
    vf = ValidationStep(m, flat, opt, xf, yv)
    assert vu.graph is not None
    for (xb, yb), nv in zip(batches, (4, 3)):
        xu.copy_(xb); xf.copy_(pn(xb)); yv.copy_(yb)
        vu.step(n_valid=nv)
        vf.step(n_valid=nv)
    torch.cuda.synchronize()
    cu, cf = vu.compute(), vf.compute()
    assert cu == cf and cu["n"] == 7
    assert torch.equal(vu.live.block, vf.live.block) and torch.equal(vu.ema_metrics.block, vf.ema_metrics.block)
    flat.close()
