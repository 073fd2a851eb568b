"""Layer-wise lr decay of the Vim baseline (``fastvim_amd.vim.VisionMamba``; mae/lr_decay.py of the reference):
``cls_token``, ``pos_embed`` and the patch projection in layer 0, block i in layer i + 1, the final norm and the head in
the last layer.  CPU only."""
import torch


def test_layer_ids_and_groups_of_the_vim_baseline():
    from fastvim_amd.lr_decay import get_layer_id_vit_vim, layer_scales, param_groups_lrd
    from fastvim_amd.vim import VisionMamba
    torch.manual_seed(0)
    depth = 4
    m = VisionMamba(img_size=64, patch_size=16, depth=depth, embed_dim=32, num_classes=10, rms_norm=True,
                    residual_in_fp32=True, fused_add_norm=True, fused_cls=True)
    L = depth + 1
    ids = {n: get_layer_id_vit_vim(n, L) for n, _ in m.named_parameters()}
    assert ids["cls_token"] == ids["pos_embed"] == ids["patch_embed.proj.weight"] == ids["patch_embed.proj.bias"] == 0
    for i in range(depth):
        block = {v for n, v in ids.items() if n.startswith(f"layers.{i}.")}
        assert block == {i + 1}, (i, block)
    assert ids["norm_f.weight"] == ids["head.weight"] == ids["head.bias"] == L
    assert set(ids.values()) == set(range(L + 1))
    groups = param_groups_lrd(m, weight_decay=0.05, no_weight_decay_list=m.no_weight_decay(), layer_decay=0.75)
    scales = layer_scales(L, 0.75)
    by_param = {id(p): g for g in groups for p in g["params"]}
    assert len(by_param) == len(ids)                                              # every parameter once
    for name, p in m.named_parameters():
        g = by_param[id(p)]
        assert g["lr_scale"] == scales[ids[name]], name
        assert g["weight_decay"] == (0.0 if (p.ndim == 1 or name in ("cls_token", "pos_embed")) else 0.05), name
