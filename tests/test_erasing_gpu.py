"""Random erasing on the device (csrc/erase.hip, the ERASE forms of csrc/unfold_u8.hip, fastvim_amd/erasing.py).

Outside the boxes every comparison is ``torch.equal``; so is every comparison between two kernels (eager against fused,
bf16 against fp32 rounded, replay against twin): the noise is ONE function (csrc/erase_noise.h) and all launches must agree
bit for bit.  Only the comparison of that function with the fp64 restatement of tests/erase_ref.py has a tolerance, because
the device's log2 / sqrt / sin / cos are the hardware's approximations: see ``NOISE_BOUND``."""
import random

import numpy as np
import pytest
import torch

import erase_ref as R

pytestmark = pytest.mark.gpu

MEAN3, STD3 = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
OUT_DTYPES = [torch.bfloat16, torch.float32]

# |device noise - fp64 reference|: the largest value MEASURED on an MI355X over the boxes of
# test_eager_fp32_against_the_fp64_reference (669 values per width; 2.913e-07 at widths 40 and 38, 2.589e-07 at 37) is
# 2.913e-07.  The bound is 4 x that = 1.165e-06, because those boxes visit only part of the functions' input range.  A
# wrong counter mapping, a swapped (cos, sin) or a neighbouring key differs by order 1.
NOISE_MEASURED = 2.913e-07
NOISE_BOUND = 4 * NOISE_MEASURED


# (4, 3, 32, W): no box / 1 x 1 / odd left and a width that is no multiple of 4 (Philox groups cut on both sides) / the
# bottom-right corner
def _edge_boxes(W):
    return [None, (7, 13, 1, 1), (5, 3, 9, 10), (20, W - 11, 12, 11)]


def _re(shape, boxes, mode="pixel", seed=11, draws=1):
    from fastvim_amd.erasing import RandomErasing
    re = RandomErasing(1.0, mode=mode, max_count=1, seed=seed).bind(shape)
    re.block("cuda")
    for _ in range(draws):                       # (advance the counter: a key other than the first)
        re.sample(rng=random.Random(0))
    re.set(boxes)
    return re


def _mask(shape, boxes):
    m = torch.zeros(shape, dtype=torch.bool)
    for b, box in enumerate(boxes):
        if box is not None:
            t, l, h, w = box
            m[b, :, t:t + h, l:l + w] = True
    return m.cuda()


def _want_noise(re, shape, boxes):
    """fp64 (B, C, H, W): the reference noise inside the boxes, 0 elsewhere."""
    out = np.zeros(shape)
    for b, box in enumerate(boxes):
        if box is not None:
            t, l, h, w = box
            out[b, :, t:t + h, l:l + w] = R.noise_box(re.key(), b, shape[1], t, l, h, w)
    return torch.from_numpy(out).cuda()


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    assert torch.equal(got, want), (got.float() - want.float()).abs().max().item()


# ---------------------------------------------------------------------------------------------- eager
@pytest.mark.parametrize("W", [40, 38, 37])          # 16-byte, 8-byte and single-element accesses
def test_eager_fp32_against_the_fp64_reference(W):
    """Measured on an MI355X: max |device - fp64| over these boxes is 2.913e-07; the bound is 4 x that, 1.165e-06
    (NOISE_MEASURED / NOISE_BOUND above; DESIGN.md section 3, *Random erasing*, quotes the same two numbers)."""
    from fastvim_amd import glue_ops as G
    shape, boxes = (4, 3, 32, W), _edge_boxes(W)
    x = torch.randn(shape, device="cuda")
    keep = x.clone()
    inside = _mask(shape, boxes)
    # const: exact zeros inside, the input's bits outside, the input untouched
    re = _re(shape, boxes, mode="const")
    got = G.random_erase(x, re.block())
    assert torch.equal(x, keep) and got.data_ptr() != x.data_ptr()
    assert torch.equal(got[~inside], x[~inside]) and not got[inside].any()
    assert int(inside.sum()) == 3 * (1 + 90 + 132)
    # pixel
    re = _re(shape, boxes, mode="pixel", draws=3)
    got = re.erase(x)
    assert torch.equal(got[~inside], x[~inside]) and torch.equal(x, keep)
    want = _want_noise(re, shape, boxes)
    err = (got.double() - want)[inside].abs().max().item()
    print(f"random_erase W={W}: max |device - fp64| = {err:.3e} over {int(inside.sum())} values (bound {NOISE_BOUND:.3e})")
    assert NOISE_BOUND <= 1e-2
    assert err <= NOISE_BOUND, err
    # (the check discriminates: the neighbouring key is a different stream)
    re.sample(rng=random.Random(0))
    re.set(boxes)
    assert (_want_noise(re, shape, boxes) - want)[inside].abs().max().item() > 1.0
    # in place: the same bits
    y = x.clone()
    re = _re(shape, boxes, mode="pixel", draws=3)
    assert re.erase(y, out=y) is y
    _same(y, got)


@pytest.mark.parametrize("W", [40, 36, 38, 37])      # bf16: 16-, 8-, 4-byte and single-element accesses
def test_eager_bf16_and_in_place_equal_the_fp32_result_rounded(W):
    shape, boxes = (4, 3, 32, W), _edge_boxes(W)
    x = torch.randn(shape, device="cuda").bfloat16()
    re = _re(shape, boxes, mode="pixel", draws=2)
    want = re.erase(x.float()).bfloat16()
    got = re.erase(x)
    _same(got, want)
    assert not torch.equal(got, x)
    y = x.clone()
    re.erase(y, out=y)
    _same(y, want)
    re = _re(shape, boxes, mode="const")
    _same(re.erase(x), torch.where(_mask(shape, boxes), torch.zeros_like(x), x))


def test_noise_properties():
    shape = (8, 3, 64, 64)
    boxes = [(1, 0, 63, 63)] * 8
    N = 8 * 3 * 63 * 63
    assert N == 95256
    x = torch.zeros(shape, device="cuda")
    re = _re(shape, boxes, mode="pixel", seed=5)
    got = re.erase(x)
    z = got[:, :, 1:, :63].double()
    assert not got[:, :, 0].any() and not got[:, :, :, 63].any()
    mean, var = z.mean().item(), z.var(unbiased=False).item()
    print(f"noise: mean {mean:.4e} (bound {5 / N ** 0.5:.4e}), var - 1 {var - 1:.4e} (bound {5 * (2 / N) ** 0.5:.4e})")
    assert abs(mean) < 5 / N ** 0.5
    assert abs(var - 1) < 5 * (2 / N) ** 0.5
    assert torch.isfinite(z).all() and z.abs().max().item() < 6.0          # |z| <= sqrt(2 * 24 ln 2) = 5.77
    # samples differ, channels differ: nowhere near equal
    assert (z[0] - z[1]).abs().mean().item() > 0.5 and (z[0, 0] - z[0, 1]).abs().mean().item() > 0.5
    assert len(torch.unique(z)) > 0.9 * N
    # two launches on one key agree bit for bit; a second sample() with the same boxes is another stream
    _same(re.erase(x), got)
    key = re.key()
    re.sample(rng=random.Random(1))
    re.set(boxes)
    again = re.erase(x)
    assert re.key() != key and (again - got)[:, :, 1:, :63].abs().mean().item() > 0.5
    # ranks pass different seeds: another stream as well
    other = _re(shape, boxes, mode="pixel", seed=6).erase(x)
    assert (other - got)[:, :, 1:, :63].abs().mean().item() > 0.5


# ---------------------------------------------------------------------------------------------- fused: plain
def _images(shape, seed, offset=0):
    """uint8 images holding every byte value; ``offset``: the view starts that many bytes into its buffer."""
    n = int(np.prod(shape))
    g = torch.Generator().manual_seed(seed)
    buf = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    x = buf[offset:offset + n].view(shape)
    x.copy_((torch.randperm(n, generator=g) % 256).to(torch.uint8).view(shape))
    assert x.is_contiguous() and x.data_ptr() % 16 == offset
    return x


# shape, patch, byte offset of the base, boxes (crossing patch and chunk boundaries, cutting Philox groups), load width
FUSED = [((4, 3, 32, 32), 16, 0, [(13, 11, 7, 10), None, (0, 0, 31, 31), (31, 15, 1, 2)], 16),
         ((4, 3, 24, 24), 8, 0, [(5, 6, 12, 11), (0, 7, 1, 1), None, (16, 13, 8, 11)], 8),
         ((2, 3, 28, 28), 14, 0, [(11, 9, 8, 13), (27, 1, 1, 26)], 4),
         ((2, 3, 16, 32), 16, 2, [(3, 13, 9, 7), (15, 30, 1, 2)], 2),
         ((2, 3, 16, 320), 16, 0, [(3, 250, 9, 13), (2, 300, 13, 19)], 16)]      # 20 patches: chunks of 16 and 4


@pytest.mark.parametrize("out_dtype", OUT_DTYPES)
@pytest.mark.parametrize("shape,patch,offset,boxes,lv", FUSED)
def test_fused_plain_equals_eager_erase_then_float_unfold(shape, patch, offset, boxes, lv, out_dtype):
    from fastvim_amd import glue_ops as G
    from fastvim_amd.pixels import PixelNorm
    pn = PixelNorm(MEAN3, STD3)
    x = _images(shape, seed=shape[2] * shape[3] + patch, offset=offset)
    assert G.patch_unfold_u8_ok(x, patch, patch)
    assert max(v for v in (16, 8, 4, 2) if shape[3] % v == 0 and (16 * patch) % v == 0 and x.data_ptr() % v == 0) == lv
    table = pn.table(x.device)
    xn = pn(x).contiguous()
    plain = G.patch_unfold_u8(x, table, patch, patch, out_dtype)
    for mode in ("pixel", "const"):
        re = _re(shape, boxes, mode=mode, draws=2)
        got = G.patch_unfold_u8_re(x, table, patch, patch, out_dtype, re.block())
        _same(got, G.patch_unfold(G.random_erase(xn, re.block()), patch, patch, out_dtype))
        assert not torch.equal(got, plain)
    # no box anywhere: the plain launch's output
    re = _re(shape, [None] * shape[0])
    _same(G.patch_unfold_u8_re(x, table, patch, patch, out_dtype, re.block()), plain)


def test_fused_noise_is_the_reference_noise():
    """The fused launch against the fp64 reference directly (fp32 patches, folded back to the image)."""
    from fastvim_amd import glue_ops as G
    from fastvim_amd.pixels import PixelNorm
    shape, patch, _, boxes, _ = FUSED[0]
    B, C, H, W = shape
    pn = PixelNorm(MEAN3, STD3)
    x = _images(shape, seed=1)
    re = _re(shape, boxes, draws=4)
    got = G.patch_unfold_u8_re(x, pn.table(x.device), patch, patch, torch.float32, re.block())
    img = got.view(B, H // patch, W // patch, C, patch, patch).permute(0, 3, 1, 4, 2, 5).reshape(shape)
    inside = _mask(shape, boxes)
    assert torch.equal(img[~inside], pn(x)[~inside])
    err = (img.double() - _want_noise(re, shape, boxes))[inside].abs().max().item()
    print(f"patch_unfold_u8_re: max |device - fp64| = {err:.3e} over {int(inside.sum())} values (bound {NOISE_BOUND:.3e})")
    assert err <= NOISE_BOUND, err


# ---------------------------------------------------------------------------------------------- fused: pairs
# The cases of FUSED at B = 4: shape, patch, byte offset of the base, erase boxes, CutMix box (yl, yh, xl, xh), load width of the
# pair kernel (8 patches per tile).  Partners are (0, 3) -- one of them without a box -- and (1, 2), two different boxes; the
# CutMix box overlaps erase boxes.  The 320-wide case has 20 patches per row, so chunks of 8, 8 and a tail of 4, with the
# erase boxes across the chunk boundaries at x = 128 and x = 256 and inside the tail.
MIX = [((4, 3, 32, 32), 16, 0, [(13, 11, 7, 10), (2, 3, 20, 9), (9, 14, 5, 17), None], (10, 20, 8, 19), 16),
       ((4, 3, 24, 24), 8, 0, [(5, 6, 12, 11), (0, 0, 9, 23), (7, 7, 10, 5), None], (10, 20, 8, 19), 8),
       ((4, 3, 28, 28), 14, 0, [(11, 9, 8, 13), (1, 2, 20, 9), (13, 12, 6, 15), None], (10, 20, 8, 19), 4),
       ((4, 3, 16, 32), 16, 2, [(3, 13, 9, 7), (15, 30, 1, 2), (0, 1, 15, 30), None], (2, 12, 5, 27), 2),
       ((4, 3, 16, 320), 16, 0, [(3, 250, 9, 13), (2, 300, 13, 19), (1, 120, 14, 21), None], (4, 13, 100, 290), 16)]


@pytest.mark.parametrize("out_dtype", OUT_DTYPES)
@pytest.mark.parametrize("shape,patch,offset,boxes,cutbox,lv", MIX)
def test_fused_mix_equals_eager_erase_then_float_mix_unfold(shape, patch, offset, boxes, cutbox, lv, out_dtype):
    from fastvim_amd import glue_ops as G
    from fastvim_amd.mixup import Mixup
    from fastvim_amd.pixels import PixelNorm
    pn = PixelNorm(MEAN3, STD3)
    x = _images(shape, seed=shape[2] + shape[3], offset=offset)
    assert G.patch_unfold_u8_ok(x, patch, patch)
    assert max(v for v in (16, 8, 4, 2) if shape[3] % v == 0 and (8 * patch) % v == 0 and x.data_ptr() % v == 0) == lv
    xn = pn(x).contiguous()
    table = pn.table(x.device)
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=10)
    mix.bind(x)
    mblock = mix.block(x.device)
    re = _re(shape, boxes, draws=2)
    outs = []
    # copy, Mixup, CutMix with a box that overlaps the erase boxes of samples 0, 1 and 2
    for lam, cut, box in ((1.0, False, None), (0.37, False, None), (0.6, True, cutbox)):
        mix.set(lam, use_cutmix=cut, box=box)
        got = G.patch_unfold_mix_u8_re(x, table, patch, patch, out_dtype, mblock, re.block())
        _same(got, G.patch_unfold_mix(G.random_erase(xn, re.block()), patch, patch, out_dtype, mblock))
        assert not torch.equal(got, G.patch_unfold_mix_u8(x, table, patch, patch, out_dtype, mblock))
        outs.append(got)
    _same(outs[0], G.patch_unfold_u8_re(x, table, patch, patch, out_dtype, re.block()))      # lam == 1: erased, not mixed
    assert not torch.equal(outs[1], outs[0]) and not torch.equal(outs[2], outs[0])
    # the module: PatchEmbed(x_u8, mix=, erase=) takes the fused launch and equals the float path on the erased batch
    from fastvim_amd.fastvim import PatchEmbed
    from fastvim_amd.pixels import attach_pixel_norm
    torch.manual_seed(0)
    pe = PatchEmbed(img_size=shape[2:], patch_size=patch, in_chans=3, embed_dim=64).cuda()
    attach_pixel_norm(pe, MEAN3, STD3)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=out_dtype == torch.bfloat16):
        _same(pe(x, mix=mix, erase=re), pe(re.erase(xn), mix=mix))
        _same(pe(x, erase=re), pe(re.erase(xn)))
        _same(pe(xn, mix=mix, erase=re), pe(re.erase(xn), mix=mix))


# ---------------------------------------------------------------------------------------------- the replayed step
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


def _batches(n=2):
    g = torch.Generator(device="cuda").manual_seed(11)
    return [(torch.randint(0, 256, (B, 3, 224, 224), device="cuda", generator=g, dtype=torch.uint8),
             torch.randint(0, CLASSES, (B,), device="cuda", generator=g)) for _ in range(n)]


def _run_step(batches, u8, erase_in_step, boxes_seed=5, no_boxes=False, probe=False):
    """Replayed steps with Mixup.  ``erase_in_step``: the step erases (``erase=re``); else, if ``boxes_seed`` is not None, the
    twin is fed ``re.erase(pn(x))``.  Returns per step (loss, boxes, gradient, parameters) and the probe's losses."""
    from fastvim_amd.erasing import RandomErasing
    from fastvim_amd.mixup import Mixup
    from fastvim_amd.pipeline import SegmentedTrainStep
    m, flat, opt, pn = _fastvim()
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=CLASSES)
    mix.set(0.5)
    x = torch.zeros(B, 3, 224, 224, device="cuda", dtype=torch.uint8 if u8 else torch.float32)
    y = torch.zeros(B, dtype=torch.int64, device="cuda")
    re = None
    if boxes_seed is not None:
        re = RandomErasing(0.6, mode="pixel", max_count=1, seed=3).bind(x)
    torch.manual_seed(7)
    step = SegmentedTrainStep(m, flat, opt, mix.criterion(), x, y, n_segments=3, use_graph=True, warmup=2, mixup=mix,
                              erase=re if erase_in_step else None)
    assert step.use_graph and step._embed_takes_mix
    if erase_in_step:
        assert step._embed_takes_erase == u8 and (step._x_erased is None) == u8
    np.random.seed(3)
    rng = random.Random(boxes_seed)
    rec, probes = [], []
    for xb, yb in batches:
        boxes = None
        if re is not None:
            boxes = re.set([None] * B) if no_boxes else re.sample(rng=rng)
        if u8:
            x.copy_(xb)
        else:
            x.copy_(pn(xb) if re is None or erase_in_step else re.erase(pn(xb)))
        y.copy_(yb)
        mix.sample()
        loss = step.step().item()
        rec.append((loss, boxes, flat.grad_flat.clone(), flat.param_flat.clone()))
    if probe:
        # lr = 0 freezes the parameters and the RNG state is put back before every replay (DropPath), so two replays differ
        # only by what the erase block holds
        opt.set_lr(0.0)
        state = torch.cuda.get_rng_state()
        for draw in (True, False, True):
            if draw:
                re.sample(rng=rng)
            torch.cuda.set_rng_state(state)
            probes.append(step.step().item())
    torch.cuda.synchronize()
    flat.close()
    return rec, probes


def test_replayed_step_erases_inside_the_uint8_unfold_like_a_float_twin_fed_the_erased_batch():
    """Three step objects, two replays each: the uint8 buffer erased inside the unfold, a float buffer erased by the step
    into its scratch batch, and a float twin that is FED ``re.erase(pn(x))`` and knows nothing of erasing."""
    batches = _batches()
    got, probes = _run_step(batches, u8=True, erase_in_step=True, probe=True)
    scratch, _ = _run_step(batches, u8=False, erase_in_step=True)
    want, _ = _run_step(batches, u8=False, erase_in_step=False)
    assert any(box != (0, 0, 0, 0) for _, boxes, _, _ in got for box in boxes)
    for other in (got, scratch):
        for (lg, bg, gg, fg), (lw, bw, gw, fw) in zip(other, want):
            assert bg == bw and lg == lw and lg == lg, (lg, lw)
            assert torch.equal(gg, gw) and torch.equal(fg, fw)
    # a replay without a fresh copy or draw is idempotent; a new sample() changes the replay
    assert probes[0] == probes[1] and probes[2] != probes[0], probes


def test_replayed_step_without_any_box_equals_the_step_built_without_erase():
    batches = _batches(n=1)
    got, _ = _run_step(batches, u8=True, erase_in_step=True, no_boxes=True)
    want, _ = _run_step(batches, u8=True, erase_in_step=False, boxes_seed=None)
    (lg, _, gg, fg), (lw, _, gw, fw) = got[0], want[0]
    assert lg == lw and torch.equal(gg, gw) and torch.equal(fg, fw)
