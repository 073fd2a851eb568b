"""CPU checks of the MAE token plan: the restatement the GPU tests compare the kernels with (tests/mae_tokens_ref.py) equals
today's torch composition and the reference's own mask, and a CPU model with ``fused_tokens`` on takes the eager path."""
import pytest
import torch

import mae_tokens_ref as R
from conftest import load_golden


@pytest.mark.parametrize("ratio", R.RATIOS)
@pytest.mark.parametrize("H,W", R.GRIDS)
def test_restatement_equals_todays_composition(H, W, ratio):
    L = H * W
    K = int(L * (1 - ratio))
    noise = R.tie_free_noise(3, L, seed=100 * H + int(100 * ratio))
    ref, eager = R.plan_ref(noise, H, W, K), R.eager_plan(noise, H, W, K)
    for k, v in eager.items():
        assert ref[k].dtype == v.dtype and torch.equal(ref[k], v), k
    # the int32 copies and the -1 form of the unshuffle index
    assert torch.equal(ref["keep_index"].long(), ref["ids_keep"]) and torch.equal(ref["order_index"].long(), ref["order"])
    assert torch.equal(ref["inverse_index"].long(), ref["inverse"])
    kept = ref["mask"] == 0
    assert torch.equal(ref["restore_index"].long()[kept], ref["ids_restore"][kept]) and bool((ref["restore_index"][~kept] == -1).all())
    assert int(kept.sum()) == 3 * K


def test_non_square_grid_equals_todays_composition():
    noise = R.tie_free_noise(2, 24, seed=7)
    ref, eager = R.plan_ref(noise, 6, 4, 6), R.eager_plan(noise, 6, 4, 6)
    for k, v in eager.items():
        assert torch.equal(ref[k], v), k


def test_tied_noise_is_the_stable_order():
    """All-equal noise keeps the first K tokens; the restatement's ranks are ``argsort(stable=True)``."""
    ref = R.plan_ref(torch.full((2, 16), 0.25), 4, 4, 4)
    assert torch.equal(ref["ids_keep"], torch.arange(4).repeat(2, 1))
    assert torch.equal(ref["ids_restore"], torch.arange(16).repeat(2, 1))


@pytest.mark.parametrize("case", ["tiny_64_keep4", "tiny_96_keep9"])
def test_restatement_mask_equals_reference_golden(case):
    c = load_golden("mae.pt")[case]
    g = c["cfg"]["img_size"] // c["cfg"]["patch_size"]
    noise = c["noise"]
    K = int(g * g * (1 - 0.75))
    assert torch.equal(R.plan_ref(noise, g, g, K)["mask"], c["mask"].float())


def test_cpu_model_with_flag_on_takes_the_eager_path():
    from fastvim_amd import mae_tokens
    from fastvim_amd.models_mae import MaskedAutoencoderViM
    torch.manual_seed(0)
    m = MaskedAutoencoderViM(img_size=64, patch_size=16, depth=2, embed_dim=32, decoder_embed_dim=32, decoder_depth=1,
                             rms_norm=True, residual_in_fp32=True, fused_add_norm=True, fused_tokens=True)
    assert m.fused_tokens is True and MaskedAutoencoderViM.fused_tokens is False
    noise = R.tie_free_noise(2, 16, seed=1)
    assert not mae_tokens.mask_plan_ok(noise, (4, 4), 4)                     # a CPU tensor
    x = torch.randn(2, 16, 32)
    xm, mask, ids_restore, ids_keep = m.random_masking(x, 0.75, noise)      # does not raise: the torch composition
    ref = R.plan_ref(noise, 4, 4, 4)
    assert torch.equal(mask, ref["mask"]) and torch.equal(ids_restore, ref["ids_restore"]) and torch.equal(ids_keep, ref["ids_keep"])
    assert torch.equal(xm, torch.gather(x, 1, ids_keep.unsqueeze(-1).expand(-1, -1, 32)))
    assert m._masking(x, 0.75, noise)[4] is None


def test_predicate_cases():
    from fastvim_amd import mae_tokens
    # CPU tensors, wrong dtype, too long, too few kept: all False without a GPU
    assert not mae_tokens.mask_plan_ok(torch.rand(2, 16), (4, 4), 4)
    assert not mae_tokens.mask_plan_ok(torch.rand(2, 16).double(), (4, 4), 4)
    assert not mae_tokens.mask_plan_ok(torch.rand(1, 33 * 33), (33, 33), 100)
    with pytest.raises(RuntimeError, match="mask_plan_ok"):
        mae_tokens.mask_plan(torch.rand(2, 16), (4, 4), 4)
