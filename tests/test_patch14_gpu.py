"""Patch width 14 (FastVim-H, MAE-H) on the patch-unfold kernels (csrc/glue.hip: fv_patch_unfold, fv_patch_unfold_mix).

14 is even but no multiple of 8: a 4-element vector of an image row straddles a patch boundary every other time and is
placed as two pairs, and the chunk of patches a workgroup writes starts on a 16-byte boundary only for some grids
(16 x 16, 32 x 32); 84 / 14 = 6 columns leave 8-byte boundaries, 42 / 14 = 3 columns an image row that is no whole number
of 4-element vectors.  Everything is a permutation and one rounding: every comparison is bit for bit."""
import copy

import pytest
import torch

from fastvim_amd.mixup import Mixup
from test_mixup_gpu import _cases, torch_mix

pytestmark = pytest.mark.gpu

DTYPES = [(torch.float32, torch.bfloat16), (torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16)]


def _permute_copy(x, ph, pw, dt):
    B, C, H, W = x.shape
    gh, gw = H // ph, W // pw
    return x.reshape(B, C, gh, ph, gw, pw).permute(0, 2, 4, 1, 3, 5).reshape(B, gh * gw, C * ph * pw).to(dt)


@pytest.mark.parametrize("in_dt,out_dt", DTYPES)
@pytest.mark.parametrize("shape", [(2, 3, 224, 224), (1, 3, 448, 448), (4, 3, 84, 84), (3, 1, 28, 42)])
def test_patch_unfold_14_equals_the_permute_copy(shape, in_dt, out_dt):
    from fastvim_amd import glue_ops as G
    torch.manual_seed(sum(shape))
    x = torch.randn(shape, device="cuda").to(in_dt)
    assert G.patch_unfold_ok(x, 14, 14)
    got = G.patch_unfold(x, 14, 14, out_dt)
    ref = _permute_copy(x, 14, 14, out_dt)
    assert got.dtype == out_dt and got.shape == ref.shape
    assert torch.equal(got, ref), (got.float() - ref.float()).abs().max().item()


@pytest.mark.parametrize("in_dt,out_dt", DTYPES)
@pytest.mark.parametrize("ph,pw", [(14, 16), (16, 14)])
def test_non_square_patches_only_the_width_decides_the_form(ph, pw, in_dt, out_dt):
    from fastvim_amd import glue_ops as G
    torch.manual_seed(ph)
    x = torch.randn(2, 3, 112, 112, device="cuda").to(in_dt)
    assert G.patch_unfold_ok(x, ph, pw)
    assert torch.equal(G.patch_unfold(x, ph, pw, out_dt), _permute_copy(x, ph, pw, out_dt))


def test_odd_patch_width_stays_rejected():
    from fastvim_amd import glue_ops as G
    x = torch.randn(2, 3, 42, 42, device="cuda")
    assert not G.patch_unfold_ok(x, 14, 7)
    with pytest.raises(RuntimeError, match="even"):
        G.patch_unfold(x, 14, 7, torch.bfloat16)


@pytest.mark.parametrize("in_dt,out_dt", DTYPES)
@pytest.mark.parametrize("shape", [(2, 3, 224, 224), (4, 3, 84, 84)])
def test_patch_unfold_mix_14_equals_unfold_of_the_mixed_batch(shape, in_dt, out_dt):
    from fastvim_amd import glue_ops as G
    torch.manual_seed(sum(shape) + 1)
    x = torch.randn(shape, device="cuda").to(in_dt)
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0)
    for name, lam, cut, box in _cases(shape[2], shape[3]):
        mix.set(lam, use_cutmix=cut, box=box)
        got = G.patch_unfold_mix(x, 14, 14, out_dt, mix.block(x.device))
        ref = G.patch_unfold(mix.mix_batch(x), 14, 14, out_dt)
        assert got.dtype == out_dt and got.shape == ref.shape
        assert torch.equal(got, ref), (name, (got.float() - ref.float()).abs().max().item())
        assert torch.equal(ref, _permute_copy(torch_mix(x, lam, cut, box), 14, 14, out_dt)), name


def test_patch_embed_14_is_the_strided_copy_path_bitwise():
    """PatchEmbed at patch 14 now unfolds through the kernel; the projection (K = 588, no multiple of 8) still takes
    LinearFn + the bias / position epilogue.  Expected value: the strided copy the parent made, fed to the same two."""
    from fastvim_amd.fastvim import LinearFn, PatchEmbed, _EmbedEpilogueFn
    torch.manual_seed(14)
    pe = PatchEmbed(img_size=84, patch_size=14, in_chans=3, embed_dim=192).cuda()
    x = torch.randn(4, 3, 84, 84, device="cuda")
    pos = torch.randn(1, 36, 192, device="cuda")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        got = pe(x, pos_embed=pos)
        patches = _permute_copy(x, 14, 14, torch.bfloat16).contiguous()
        ref = _EmbedEpilogueFn.apply(LinearFn.apply(patches, pe.proj.weight, torch.bfloat16), pe.proj.bias, pos)
    assert got.dtype == ref.dtype and torch.equal(got, ref)


def test_h_model_step_with_mixup_replays_bitwise_and_issues_no_mix_batch(monkeypatch):
    """FastVim-H geometry (embed 1280, patch 14, 16 x 16 grid), depth 2, Mixup inside SegmentedTrainStep: the replayed
    step equals the eager step bit for bit, and the mixing happens inside the unfold launch -- ``glue_ops.mix_batch``
    raises while the steps are built and run."""
    from fastvim_amd import glue_ops as G
    from fastvim_amd.fastvim import VisionMamba
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    from fastvim_amd.pipeline import SegmentedTrainStep
    B, C = 4, 10
    torch.manual_seed(0)
    base = VisionMamba(embed_dim=1280, depth=2, img_size=224, patch_size=14, stride=14, num_classes=C, drop_path_rate=0.0,
                       rms_norm=True, residual_in_fp32=True, fused_add_norm=True, final_pool_type="mean",
                       if_abs_pos_embed=True).cuda().train()
    gen = torch.Generator(device="cuda").manual_seed(11)
    xb = torch.randn(B, 3, 224, 224, device="cuda", generator=gen)
    yb = torch.randint(0, C, (B,), device="cuda", generator=gen)

    def no_mix_batch(*a, **k):
        raise AssertionError("fv_mix_batch issued: patch 14 must mix inside the unfold kernel")
    monkeypatch.setattr(G, "mix_batch", no_mix_batch)

    def run(use_graph):
        m = copy.deepcopy(base)
        flat = FlatTrainingState(m)
        opt = FlatAdamW(flat, m, lr=1e-3, weight_decay=0.05, ema_decay=0.999)
        mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=C)
        mix.set(0.5)
        x, y = xb.clone(), yb.clone()
        torch.manual_seed(7)
        step = SegmentedTrainStep(m, flat, opt, mix.criterion(), x, y, n_segments=2, use_graph=use_graph, warmup=2, mixup=mix)
        assert step.use_graph is use_graph
        mix.set(0.71, use_cutmix=True, box=(40, 150, 0, 97))
        loss = step.step().item()
        torch.cuda.synchronize()
        out = (loss, flat.param_flat.clone(), opt.ema.clone())
        flat.close()
        return out

    g, e = run(True), run(False)
    assert g[0] == g[0] and abs(g[0]) < 1e4
    assert g[0] == e[0] and torch.equal(g[1], e[1]) and torch.equal(g[2], e[2])
