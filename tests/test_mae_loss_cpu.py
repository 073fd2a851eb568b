"""CPU-side checks of the fused MAE reconstruction loss: the fp64 restatement the GPU tests compare against IS the model's
``forward_loss``; the C ABI declares and exports the new entry points; the host predicates accept and reject the listed
shapes; a CPU uint8 batch takes the lookup fallback."""
import ctypes
import os
import re

import pytest
import torch

import mae_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(img=32, patch=16, **kw):
    from fastvim_amd.models_mae import MaskedAutoencoderViM
    return MaskedAutoencoderViM(img_size=img, patch_size=patch, depth=1, embed_dim=64, decoder_embed_dim=64, decoder_depth=1,
                                rms_norm=True, residual_in_fp32=True, fused_add_norm=True, **kw)


@pytest.mark.parametrize("norm_pix", [True, False])
@pytest.mark.parametrize("patch,px,N", [(16, 48, 3), (14, 28, 2), (8, 16, 2)])
def test_restatement_equals_forward_loss_in_fp64(patch, px, N, norm_pix):
    c = R.make_case(patch, px, N)
    m = _model(px, patch, norm_pix_loss=norm_pix)
    mask = R.make_mask("ratio75", N, c["pred"].shape[1])
    img, pred = c["f32"].double(), c["pred"].double().requires_grad_(True)
    loss = m.forward_loss(img, pred, mask.double())
    loss.backward()
    ref = R.mae_loss_ref(c["f32"], c["pred"], mask, patch, norm_pix)
    assert abs(loss.item() - ref["loss"].item()) <= 1e-13 * abs(ref["loss"].item())
    assert (pred.grad - ref["dpred"]).abs().max().item() <= 1e-13 * ref["dpred"].abs().max().item()
    assert torch.equal(R.patch_targets(c["f32"], patch), m.patchify(c["f32"].double()))
    # the upstream gradient scales dpred
    half = R.mae_loss_ref(c["f32"], c["pred"], mask, patch, norm_pix, g=0.5)
    assert torch.equal(half["dpred"], ref["dpred"] * 0.5)


def test_symbols_are_declared_exported_and_the_abi_version_stays():
    from fastvim_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fastvim_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.lib()
    for s in ("fv_mae_loss_ok", "fv_mae_loss_fwd", "fv_mae_loss_bwd"):
        assert re.search(r"\bint\s+%s\s*\(" % s, code), s
        assert s in _lib.C_ABI_SYMBOLS
        assert hasattr(lib, s), s
    assert "fv_mae_loss_ok, fv_mae_loss_fwd and fv_mae_loss_bwd were ADDED" in hdr
    assert int(re.search(r"#define\s+FV_ABI_VERSION\s+(\d+)", hdr).group(1)) == 3 == lib.fv_version()
    assert os.path.exists(os.path.join(ROOT, "fastvim_amd", "csrc", "mae_loss.hip"))


#          batch, chans, height, width, patch, pred dtype code -> accepted
SHAPE_RULES = [
    ((128, 3, 224, 224, 16, 0), True), ((128, 3, 224, 224, 16, 1), True), ((128, 3, 224, 224, 14, 1), True),
    ((1, 3, 448, 448, 14, 0), True), ((2, 3, 16, 16, 8, 1), True), ((3, 3, 48, 48, 16, 0), True), ((4, 3, 56, 56, 28, 1), True),
    ((128, 3, 448, 448, 14, 1), True),                                     # 128 x 1024 patches: the limit itself
    ((129, 3, 448, 448, 14, 1), False),                                    # one image past it
    ((2, 1, 32, 32, 16, 0), False), ((2, 4, 32, 32, 16, 0), False),        # channels != 3
    ((2, 3, 32, 48, 16, 0), False),                                        # not square
    ((2, 3, 40, 40, 16, 0), False),                                        # ragged
    ((2, 3, 30, 30, 15, 0), False), ((2, 3, 12, 12, 6, 0), False), ((2, 3, 64, 64, 32, 0), False),      # patch odd, < 8, > 28
    ((2, 3, 32, 32, 16, 2), False),                                        # fp16 pred
    ((0, 3, 32, 32, 16, 0), False),
]


def test_host_predicate_accepts_and_rejects_the_listed_shapes():
    """``fv_mae_loss_ok`` is host code; the Python predicate applies the same shape rule."""
    from fastvim_amd import _lib
    lib = _lib.lib()
    dts = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
    for args, want in SHAPE_RULES:
        assert bool(lib.fv_mae_loss_ok(*(ctypes.c_int(a) for a in args))) is want, args
        B, C, H, W, p, dt = args
        assert _python_shape_rule(B, C, H, W, p, dts[dt]) is want, args


def _python_shape_rule(B, C, H, W, p, dt):
    """The shape part of ``mae_reconstruction_loss_ok``: asked with CPU tensors it always says no (a CPU batch falls back), so
    the shape rule is isolated by pretending the tensors are on the GPU."""
    from fastvim_amd.losses import mae_reconstruction_loss_ok

    class _OnGpu:
        def __init__(self, shape, dtype):
            self.shape, self.dtype, self.device, self.is_cuda, self.requires_grad = torch.Size(shape), dtype, "gpu", True, False

        def dim(self):
            return len(self.shape)

        def is_contiguous(self):
            return True

    Lp = (H // p) * (W // p) if p > 0 else 0
    return mae_reconstruction_loss_ok(_OnGpu((B, C, H, W), torch.float32), _OnGpu((B, Lp, 3 * p * p), dt),
                                      _OnGpu((B, Lp), torch.float32), p)


def test_python_predicate_rejects_what_only_the_host_sees():
    from fastvim_amd.losses import mae_reconstruction_loss, mae_reconstruction_loss_ok
    c = R.make_case(16, 32, 2)
    mask = R.make_mask("ratio75", 2, 4)
    assert not mae_reconstruction_loss_ok(c["f32"], c["pred"], mask, 16)                     # CPU tensors
    assert not mae_reconstruction_loss_ok(c["u8"], c["pred"], mask, 16, c["table"])
    with pytest.raises(RuntimeError, match="unsupported"):
        mae_reconstruction_loss(c["f32"], c["pred"], mask, 16)


def test_cpu_uint8_batch_takes_the_lookup_fallback_bit_for_bit():
    from fastvim_amd.pixels import IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD, attach_pixel_norm, pixel_table
    c = R.make_case(16, 32, 2)
    mask = R.make_mask("ratio75", 2, 4)
    for norm_pix in (True, False):
        m = _model(32, 16, norm_pix_loss=norm_pix)
        pn = attach_pixel_norm(m, IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD)
        table = pixel_table(m.patch_embed, c["u8"])
        got = m.reconstruction_loss(c["u8"], c["pred"], mask, table)
        assert torch.equal(got, m.forward_loss(pn(c["u8"]), c["pred"], mask))
        m.fused_loss = True               # float CPU images: the predicate says no, the composition runs
        assert torch.equal(m.reconstruction_loss(pn(c["u8"]), c["pred"], mask), m.forward_loss(pn(c["u8"]), c["pred"], mask))


def test_fused_loss_keyword_and_attribute():
    from fastvim_amd import fastvim_mae
    m = _model()
    assert m.fused_loss is False
    assert _model(fused_loss=True).fused_loss is True
    m.fused_loss = True
    assert m.fused_loss is True
    v = fastvim_mae.MaskedAutoencoderViM(img_size=32, depth=1, embed_dim=64, decoder_embed_dim=64, decoder_depth=1, rms_norm=True,
                                         residual_in_fp32=True, fused_add_norm=True, fused_loss=True)
    assert v.fused_loss is True and "fused_loss" not in v.state_dict()


def test_uint8_without_a_table_is_refused_before_anything_runs():
    m = _model()
    with pytest.raises(TypeError, match="attach_pixel_norm"):
        m(torch.zeros(2, 3, 32, 32, dtype=torch.uint8))
