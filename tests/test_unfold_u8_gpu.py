"""The uint8 patch-unfold kernels (csrc/unfold_u8.hip) against "normalise, then the float kernel", bit for bit.

The reference of every comparison is ``existing float function(PixelNorm(x_u8))`` and every comparison is ``torch.equal``.
Images are ``randperm(H * W) % 256`` per channel, so every byte value -- the ones from 128 up, where a sign extension
would show, included -- occurs in every channel (the smallest plane here, 24 x 40, holds all 256).  The shapes are the
smallest that reach each way of going wrong: more than one chunk of 16 patches with a tail of one, every load width
(16, 8, 4 and 2 bytes, by row stride and by base address), patch widths 16, 8 and 14, both output types."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MEAN3, STD3 = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
MEAN8 = (0.0913, 0.1377, 0.2048, 0.0562, 0.3301, 0.4419, 0.0271, 0.1802)
STD8 = (0.0721, 0.1139, 0.1618, 0.0333, 0.2504, 0.2987, 0.0119, 0.0906)
OUT_DTYPES = [torch.bfloat16, torch.float32]


def _images(shape, seed):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.stack([torch.stack([(torch.randperm(H * W, generator=g) % 256).view(H, W) for _ in range(C)]) for _ in range(B)])
    x = x.to(torch.uint8)
    assert all(len(torch.unique(x[b, c])) == 256 for b in range(B) for c in range(C))
    return x.cuda()


def _norm(C):
    from fastvim_amd.pixels import PixelNorm
    return PixelNorm(MEAN3, STD3) if C == 3 else PixelNorm(MEAN8, STD8)


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    assert torch.equal(got, want), (got.float() - want.float()).abs().max().item()


# ---------------------------------------------------------------------------------------------- plain
PLAIN = [((2, 3, 32, 48), 16, None),       # non-square, 3 patches per row
         ((2, 3, 16, 272), 16, None),      # 17 patches: crosses the 16-patch chunk, tail of one
         ((2, 3, 24, 40), 8, None),        # row stride 40 B: 8-byte loads
         ((2, 3, 28, 112), 14, None),      # the FastVim-H form, 16-byte-aligned rows, pairs placed
         ((2, 3, 28, 42), 14, None),       # row stride 42 B: 2-byte loads
         ((3, 3, 28, 42), 14, 1)]          # x[1:]: the base is 8 bytes off a 16-byte boundary


@pytest.mark.parametrize("out_dtype", OUT_DTYPES)
@pytest.mark.parametrize("shape,patch,first", PLAIN)
def test_plain_equals_normalise_then_float_kernel(shape, patch, first, out_dtype):
    from fastvim_amd import glue_ops as G
    pn = _norm(3)
    x = _images(shape, seed=shape[2] * shape[3] + patch)
    if first is not None:
        x = x[first:]
        assert x.is_contiguous() and x.data_ptr() % 16 != 0
    table = pn.table(x.device)
    want = G.patch_unfold(pn(x).contiguous(), patch, patch, out_dtype)
    if G.patch_unfold_u8_ok(x, patch, patch):
        _same(G.patch_unfold_u8(x, table, patch, patch, out_dtype), want)
    # the module's branch: the kernel where the predicate says so, else the eager lookup and the float path -- same values
    from fastvim_amd.fastvim import PatchEmbed
    from fastvim_amd.pixels import attach_pixel_norm
    torch.manual_seed(0)
    pe = PatchEmbed(img_size=shape[2:], patch_size=patch, in_chans=3, embed_dim=64, strict_img_size=False).cuda()
    attach_pixel_norm(pe, MEAN3, STD3)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=out_dtype == torch.bfloat16):
        _same(pe(x), pe(pn(x)))


def test_predicate_accepts_every_plain_case():
    """None of the cases above is served by the fallback: the 2-byte-stride and the misaligned-base forms are kernels."""
    from fastvim_amd import glue_ops as G
    for shape, patch, first in PLAIN:
        x = torch.empty(shape, dtype=torch.uint8, device="cuda")
        assert G.patch_unfold_u8_ok(x if first is None else x[first:], patch, patch), (shape, patch)
    cl = torch.empty(2, 3, 32, 48, dtype=torch.uint8, device="cuda").contiguous(memory_format=torch.channels_last)
    assert not G.patch_unfold_u8_ok(cl, 16, 16)


# ---------------------------------------------------------------------------------------------- mix
def _draws(H, W, patch):
    """Mixup.sample() under fixed numpy seeds until mixup, a cutmix box cutting through patches, a cutmix box touching the
    border and "off" have each occurred: the parameter sets, drawn on the host."""
    from fastvim_amd.mixup import Mixup
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.7, label_smoothing=0.1, num_classes=10)
    mix.bind((H, W))
    seen, out = set(), []
    for seed in range(200):
        np.random.seed(seed)
        lam, cut, (yl, yh, xl, xh) = mix.sample()
        if lam == 1.0:
            kind = "off"
        elif not cut:
            kind = "mixup"
        elif yh > yl and xh > xl and (yl == 0 or xl == 0 or yh == H or xh == W):
            kind = "cutmix_border"
        elif yh > yl and xh > xl and (yl % patch or yh % patch) and (xl % patch or xh % patch):
            kind = "cutmix_through"
        else:
            continue
        if kind not in seen:
            seen.add(kind)
            out.append((kind, lam, cut, (yl, yh, xl, xh)))
        if len(seen) == 4:
            break
    assert seen == {"off", "mixup", "cutmix_border", "cutmix_through"}, seen
    return mix, out


@pytest.mark.parametrize("out_dtype", OUT_DTYPES)
@pytest.mark.parametrize("shape,patch", [((4, 3, 32, 48), 16), ((4, 3, 28, 112), 14)])
def test_mix_equals_normalise_then_float_mix_kernel(shape, patch, out_dtype):
    from fastvim_amd import glue_ops as G
    pn = _norm(3)
    x = _images(shape, seed=5 + patch)
    xn = pn(x).contiguous()
    table = pn.table(x.device)
    assert G.patch_unfold_u8_ok(x, patch, patch)
    mix, draws = _draws(shape[2], shape[3], patch)
    block = mix.block(x.device)
    outs = []
    for kind, lam, cut, box in draws:
        mix.set(lam, use_cutmix=cut, box=box if cut else None)
        got = G.patch_unfold_mix_u8(x, table, patch, patch, out_dtype, block)
        _same(got, G.patch_unfold_mix(xn, patch, patch, out_dtype, block))
        outs.append(got)
    # (the four parameter sets really mixed differently)
    off = [o for (kind, *_), o in zip(draws, outs) if kind == "off"][0]
    _same(off, G.patch_unfold_u8(x, table, patch, patch, out_dtype))
    assert all(not torch.equal(o, off) for (kind, *_), o in zip(draws, outs) if kind != "off")


# ---------------------------------------------------------------------------------------------- per channel
@pytest.mark.parametrize("out_dtype", OUT_DTYPES)
@pytest.mark.parametrize("colwise", [False, True])
@pytest.mark.parametrize("patch", [16, 8])
def test_chan_equals_normalise_then_float_chan_kernel(patch, colwise, out_dtype):
    from fastvim_amd import glue_ops as G
    pn = _norm(8)
    x = _images((2, 8, 32, 32), seed=patch)
    xn = pn(x).contiguous()
    table = pn.table(x.device)
    for channels in (list(range(8)), [1, 4, 6], [7]):
        n = len(channels)
        assert G.patch_unfold_chan_u8_ok(x, patch, patch, n)
        sel = torch.tensor(channels, dtype=torch.int32, device="cuda")
        got = G.patch_unfold_chan_u8(x, table, patch, patch, out_dtype, sel, n, colwise=colwise)
        _same(got, G.patch_unfold_chan(xn, patch, patch, out_dtype, sel, n, colwise=colwise))
    # no index array: the first n channels, each by its own row of the table
    _same(G.patch_unfold_chan_u8(x, table, patch, patch, out_dtype, None, 3, colwise=colwise),
          G.patch_unfold_chan(xn, patch, patch, out_dtype, None, 3, colwise=colwise))
    # an index outside the image, written into the device array, is clamped -- image channel AND table row -- like the float kernel's
    sel = torch.tensor([-3, 4, 77], dtype=torch.int32, device="cuda")
    got = G.patch_unfold_chan_u8(x, table, patch, patch, out_dtype, sel, 3, colwise=colwise)
    _same(got, G.patch_unfold_chan(xn, patch, patch, out_dtype, sel, 3, colwise=colwise))
    _same(got, G.patch_unfold_chan(xn, patch, patch, out_dtype, torch.tensor([0, 4, 7], dtype=torch.int32, device="cuda"), 3,
                                   colwise=colwise))
