"""Layer-wise lr-decay groups (fastvim_amd/lr_decay.py) against the reference's mae/lr_decay.py -- recorded as names and
numbers in tests/golden/lr_decay.json by tests/golden/gen_lr_decay.py -- and against the closed form."""
import json
import math
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


class _ToyViT(torch.nn.Module):
    """The parameter names a ViT has (``blocks``), nothing more."""

    def __init__(self, depth=5, dim=8):
        super().__init__()
        self.cls_token = torch.nn.Parameter(torch.zeros(1, 1, dim))
        self.pos_embed = torch.nn.Parameter(torch.zeros(1, 5, dim))
        self.patch_embed = torch.nn.Conv2d(3, dim, 4, 4)
        self.blocks = torch.nn.ModuleList(
            torch.nn.Sequential(torch.nn.LayerNorm(dim), torch.nn.Linear(dim, dim)) for _ in range(depth))
        self.frozen = torch.nn.Parameter(torch.zeros(3, 3), requires_grad=False)
        self.norm = torch.nn.LayerNorm(dim)
        self.head = torch.nn.Linear(dim, 3)


def _vim(depth):
    from fastvim_amd.fastvim import VisionMamba
    return VisionMamba(img_size=32, patch_size=16, depth=depth, embed_dim=16, channels=3, num_classes=5, rms_norm=True,
                       residual_in_fp32=True, fused_add_norm=True, final_pool_type="mean", if_abs_pos_embed=True)


# case name -> (model builder, keyword arguments of param_groups_lrd; "no_weight_decay_list": None = model.no_weight_decay())
CASES = {
    "vim_depth3_d075": (lambda: _vim(3), dict(weight_decay=0.05, layer_decay=0.75, arch="vim", no_weight_decay_list=None)),
    "vim_depth4_d065": (lambda: _vim(4), dict(weight_decay=0.1, layer_decay=0.65, arch="vim", no_weight_decay_list=None)),
    "vim_depth24_d075": (lambda: _vim(24), dict(weight_decay=0.05, layer_decay=0.75, arch="vim", no_weight_decay_list=None)),
    "vim_depth24_nolist": (lambda: _vim(24), dict(weight_decay=0.05, layer_decay=0.75, arch="vim", no_weight_decay_list=[])),
    "vit_depth5_d065": (lambda: _ToyViT(5), dict(weight_decay=0.05, layer_decay=0.65, arch="vit",
                                                 no_weight_decay_list=["pos_embed", "cls_token", "head.weight"])),
}


def build_case(name):
    torch.manual_seed(0)
    make, kw = CASES[name]
    model = make()
    kw = dict(kw)
    if kw["no_weight_decay_list"] is None:
        kw["no_weight_decay_list"] = sorted(model.no_weight_decay())
    return model, kw


def named_groups(model, groups):
    name_of = {id(p): n for n, p in model.named_parameters()}
    return [{"lr_scale": g["lr_scale"], "weight_decay": g["weight_decay"], "params": [name_of[id(p)] for p in g["params"]]}
            for g in groups]


def _golden():
    with open(os.path.join(HERE, "golden", "lr_decay.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("case", sorted(CASES))
def test_param_groups_lrd_matches_reference_recording(case):
    from fastvim_amd.lr_decay import param_groups_lrd
    model, kw = build_case(case)
    got = named_groups(model, param_groups_lrd(model, **kw))
    rec = _golden()[case]
    assert rec["kwargs"] == kw
    exp = rec["groups"]
    assert [g["params"] for g in got] == [g["params"] for g in exp]            # membership and order
    for g, e in zip(got, exp):
        assert g["weight_decay"] == e["weight_decay"]
        assert abs(g["lr_scale"] - e["lr_scale"]) <= 1e-12 * e["lr_scale"]


@pytest.mark.parametrize("case", sorted(CASES))
def test_param_groups_lrd_closed_form(case):
    from fastvim_amd.lr_decay import get_layer_id_vit_vim, param_groups_lrd
    model, kw = build_case(case)
    d, arch = kw["layer_decay"], kw["arch"]
    L = len(model.blocks if arch == "vit" else model.layers) + 1
    groups = named_groups(model, param_groups_lrd(model, **kw))
    trainable = [n for n, p in model.named_parameters() if p.requires_grad]
    assert sorted(n for g in groups for n in g["params"]) == sorted(trainable)      # each exactly once, frozen ones left out
    shapes = dict(model.named_parameters())
    seen = []
    for g in groups:
        ids = {get_layer_id_vit_vim(n, L) for n in g["params"]}
        assert len(ids) == 1
        i = ids.pop()
        if arch == "vit":
            expo = L - i
        else:
            expo = math.ceil(L / 2) if i == 0 else math.ceil((L - i) / 2)
        assert abs(g["lr_scale"] - d ** expo) <= 1e-12 * d ** expo
        undecayed = {shapes[n].ndim == 1 or n in kw["no_weight_decay_list"] for n in g["params"]}
        assert len(undecayed) == 1
        assert g["weight_decay"] == (0.0 if undecayed.pop() else kw["weight_decay"])
        seen.append((i, g["weight_decay"] != 0.0))
    assert len(set(seen)) == len(seen)                                              # one group per (layer id, decayed)
    first = {}
    for n in trainable:                                                              # first-seen order
        key = (get_layer_id_vit_vim(n, L), not (shapes[n].ndim == 1 or n in kw["no_weight_decay_list"]))
        first.setdefault(key, len(first))
    assert seen == sorted(seen, key=lambda k: first[k])


def test_layer_ids_and_depth24_exponents():
    from fastvim_amd.lr_decay import get_layer_id_vit_vim, param_groups_lrd
    assert get_layer_id_vit_vim("cls_token", 25) == 0 and get_layer_id_vit_vim("pos_embed", 25) == 0
    assert get_layer_id_vit_vim("patch_embed.proj.weight", 25) == 0
    assert get_layer_id_vit_vim("layers.7.mixer.A_log", 25) == 8 and get_layer_id_vit_vim("blocks.0.attn.qkv.weight", 13) == 1
    assert get_layer_id_vit_vim("norm_f.weight", 25) == 25 and get_layer_id_vit_vim("head.bias", 25) == 25
    model, kw = build_case("vim_depth24_d075")
    groups = param_groups_lrd(model, **kw)
    expo = [round(math.log(g["lr_scale"]) / math.log(0.75)) for g in groups]
    # L = 25: the embedding at ceil(25 / 2) = 13, blocks 1 .. 24 at 12, 12, 11, 11, ..., 1, 1 (a decayed and an un-decayed
    # group each), norm_f / head at 0
    assert sorted(expo, reverse=True) == [13, 13] + [e for e in range(12, 0, -1) for _ in range(4)] + [0, 0]
    with pytest.raises(ValueError):
        param_groups_lrd(model, arch="swin")
