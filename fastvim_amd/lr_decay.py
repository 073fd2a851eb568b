"""Layer-wise learning-rate decay groups for fine-tuning (drop-in for the reference's ``mae/lr_decay.py``).

``param_groups_lrd`` returns torch-style parameter groups, each with an ``lr_scale`` the training loop multiplies the
scheduled lr by (mae/finetune_imagenet.py:148-151).  ``FlatAdamW(..., param_groups=param_groups_lrd(...))`` takes them
unchanged and applies the scale on the device (fastvim_amd/flat.py, csrc/optim.hip).

Layer ids: 0 for ``cls_token`` / ``pos_embed`` / ``patch_embed*``, ``i + 1`` for ``layers.i.*`` / ``blocks.i.*``, and
``L = number of blocks + 1`` for everything else (final norm, head).  With decay ``d``:

* ``arch="vit"``: id ``i`` trains at ``d ** (L - i)``;
* ``arch="vim"``: a Vim / FastVim stack has twice the layers of the ViT of the same size, so the exponent moves every
  second layer: id 0 at ``d ** ceil(L / 2)``, id ``i >= 1`` at ``d ** ceil((L - i) / 2)``.
"""


def get_layer_id_vit_vim(name, num_layers):
    """Layer id of the parameter called ``name``; ``num_layers`` = number of blocks + 1."""
    if name in ("cls_token", "pos_embed") or name.startswith("patch_embed"):
        return 0
    if name.startswith("blocks") or name.startswith("layers"):
        return int(name.split(".")[1]) + 1
    return num_layers


def layer_scales(num_layers, layer_decay, arch="vim"):
    """``lr_scale`` of layer ids ``0 .. num_layers``."""
    if arch == "vit":
        return [layer_decay ** (num_layers - i) for i in range(num_layers + 1)]
    if arch == "vim":
        half_up = lambda k: (k + 1) // 2
        return [layer_decay ** half_up(num_layers)] + [layer_decay ** half_up(num_layers - i) for i in range(1, num_layers + 1)]
    raise ValueError(f"param_groups_lrd: arch must be 'vim' or 'vit', got {arch!r}")


def param_groups_lrd(model, weight_decay=0.05, no_weight_decay_list=[], layer_decay=0.75, arch="vim"):
    """Parameter groups keyed by (layer id, decayed or not), in first-seen order of ``model.named_parameters()``: a list
    of ``{"lr_scale", "weight_decay", "params"}``.  A parameter is left un-decayed when it is one-dimensional or named in
    ``no_weight_decay_list``; parameters that do not require a gradient are left out."""
    num_layers = len(model.blocks if arch == "vit" else model.layers) + 1
    scales = layer_scales(num_layers, layer_decay, arch)
    groups = {}
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        decayed = not (p.ndim == 1 or name in no_weight_decay_list)
        layer_id = get_layer_id_vit_vim(name, num_layers)
        key = (layer_id, decayed)
        if key not in groups:
            groups[key] = {"lr_scale": scales[layer_id], "weight_decay": weight_decay if decayed else 0.0, "params": []}
        groups[key]["params"].append(p)
    return list(groups.values())
