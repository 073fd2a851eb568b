"""CPU-side checks of the dense-prediction work: the recorded reference data is complete, ``fastvim_amd.vitdet.LN2d``
mirrors the reference class, and the host-only partial-row queries of the C ABI describe the buffers Python allocates."""
import ctypes

import pytest
import torch

from conftest import load_golden
from dense_recipe import LN2D_SHAPES, checksum, ln2d_inputs, seeded_randn

TAP_SHAPES = [(B, H, W, C) for C in (192, 384, 768) for (B, H, W) in ((2, 4, 6), (2, 5, 7), (1, 1, 1), (2, 32, 32))]


def test_dense_fixture_is_complete():
    d = load_golden("dense.pt")
    assert set(d["models"]) == {"t_64x96", "s_80x112"}
    for name, (img, dim, depth, idx) in {"t_64x96": ((64, 96), 192, 4, [1, 3]), "s_80x112": ((80, 112), 384, 2, [0, 1])}.items():
        c = d["models"][name]
        kw = c["model_kwargs"]
        assert (tuple(kw["img_size"]), kw["embed_dim"], kw["depth"], kw["out_indices"]) == (img, dim, depth, idx)
        assert (kw["rms_norm"], kw["fused_add_norm"], kw["residual_in_fp32"], kw["final_pool_type"]) == (False, False, True, "all")
        assert kw["if_abs_pos_embed"] and kw["rotate_every_block"] and kw["drop_path_rate"] == 0.0 and c["batch"] == 2
        # the image and the cotangents are rebuilt from their seeds: the recipe must reproduce what was recorded
        x = seeded_randn(c["x_seed"], 2, 3, *img)
        assert checksum(x) == pytest.approx(c["x_checksum"], rel=1e-12)
        t = load_golden(c["tensors_file"])
        gh, gw = img[0] // 16, img[1] // 16
        assert [tuple(o.shape) for o in t["outs"]] == [(2, dim, gh, gw)] * 2 and t["outs"][0].dtype == torch.float64
        want = {"x", "pos_embed", "outnorm_0.weight", "outnorm_0.bias", "outnorm_1.weight", "outnorm_1.bias",
                "layers.0.norm.weight", "layers.0.norm.bias", f"layers.{depth - 1}.norm.weight", f"layers.{depth - 1}.norm.bias"}
        assert set(t["grads"]) == want == set(c["err_ref32"]) == set(c["grad_names"])
        assert all(g.dtype == torch.float64 for g in t["grads"].values())
        assert all(0 < e < 1e-3 for e in c["err_ref32"].values())
    ln = d["ln2d"]
    maps = load_golden(ln["maps_file"])
    assert set(ln["cases"]) == set(maps) == set(LN2D_SHAPES)
    for shape in LN2D_SHAPES:
        N, C, H, W = shape
        rec, mp = ln["cases"][shape], maps[shape]
        x, dy, w, b = ln2d_inputs(shape, rec["seed"])
        assert checksum(x) == pytest.approx(rec["x_checksum"], rel=1e-12)
        assert checksum(dy) == pytest.approx(rec["dy_checksum"], rel=1e-12)
        assert torch.equal(x, x.bfloat16().float()) and torch.equal(w, w.bfloat16().float())     # one record serves fp32 and bf16
        n_y = N * H * W if rec["rows"] is None else len(rec["rows"])
        n_dx = N * H * W if rec["dx_rows"] is None else len(rec["dx_rows"])
        assert mp["y_rows"].shape == (n_y, C) and mp["dx_rows"].shape == (n_dx, C) and mp["y_rows"].dtype == torch.float64
        assert rec["dw"].shape == (C,) and rec["db"].shape == (C,)
        # the recorded output is the formula of the issue: weight * (x - mean_c) / sqrt(var_c + eps) + bias
        xr = x.double().permute(0, 2, 3, 1).reshape(-1, C)
        mu = xr.mean(1, keepdim=True)
        y = (xr - mu) / torch.sqrt((xr - mu).square().mean(1, keepdim=True) + ln["eps"]) * w.double() + b.double()
        y = y if rec["rows"] is None else y[rec["rows"]]
        assert (y - mp["y_rows"]).abs().max().item() <= 1e-12 * max(1.0, y.abs().max().item())


def test_ln2d_module_mirrors_the_reference_class():
    from fastvim_amd.vitdet import LN2d
    ln = load_golden("dense.pt")["ln2d"]
    m = LN2d(96)
    assert list(m.state_dict().keys()) == ln["state_dict_keys"] == ["weight", "bias"]
    assert m.eps == ln["eps"] == 1e-6
    assert m.normalized_shape == (96,)
    assert torch.equal(m.weight.detach(), torch.ones(96)) and torch.equal(m.bias.detach(), torch.zeros(96))
    assert isinstance(m.weight, torch.nn.Parameter) and isinstance(m.bias, torch.nn.Parameter)
    assert LN2d(256, eps=1e-5).eps == 1e-5


def test_dense_ops_have_no_cpu_fallback():
    from fastvim_amd.dense_ops import ln2d_fn, tap_layer_norm_nchw
    from fastvim_amd.vitdet import LN2d
    with pytest.raises(RuntimeError, match="GPU only"):
        tap_layer_norm_nchw(torch.randn(1, 6, 192), torch.ones(192), torch.zeros(192), 2, 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        ln2d_fn(torch.randn(1, 96, 2, 3), torch.ones(96), torch.zeros(96))
    with pytest.raises(RuntimeError, match="GPU only"):
        LN2d(96)(torch.randn(1, 96, 2, 3))


def test_partial_row_queries():
    """fv_tap_ln_blocks / fv_ln2d_blocks are plain host code: positive for every shape of the GPU tests (the row counts of
    the partial_dw / partial_db buffers), one row per workgroup, 0 for what the launches refuse."""
    from fastvim_amd import _lib
    lib = _lib.lib()
    i = ctypes.c_int
    for (B, H, W, C) in TAP_SHAPES:
        assert lib.fv_tap_ln_blocks(i(B), i(H * W)) == B * -(-(H * W) // 32) > 0
    assert lib.fv_tap_ln_blocks(i(2), i(4096)) == 256 and lib.fv_tap_ln_blocks(i(0), i(4)) == 0
    for (N, C, H, W) in LN2D_SHAPES:
        nb = lib.fv_ln2d_blocks(i(N), i(C), i(H * W))
        assert nb > 0 and nb % N == 0
        assert -(-(H * W) // 64) <= nb // N <= -(-(H * W) // 16)         # tiles of 16 to 64 positions
    assert lib.fv_ln2d_blocks(i(2), i(256), i(65536)) == 2 * 65536 // 32      # two 256 x 32 fp32 tiles: 64 KiB
    assert lib.fv_ln2d_blocks(i(1024), i(256), i(49)) == 2048                  # RoI maps: tiles of 32 and 17 positions
    assert lib.fv_ln2d_blocks(i(2), i(0), i(4)) == 0 and lib.fv_ln2d_blocks(i(2), i(1025), i(4)) == 0
