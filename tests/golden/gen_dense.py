"""Record what the reference computes on the dense-prediction path, for ``tests/test_dense_cpu.py``,
``tests/test_dense_ops_gpu.py`` and ``tests/test_dense_model_gpu.py`` (build container only: it imports the reference by
path).

    python tests/golden/gen_dense.py

Writes ``dense.pt`` next to this file, and -- no committed file may exceed 1 MiB -- the large tensors it describes into
``dense_<model case>.pt`` and ``dense_ln2d.pt``:

``dense.pt``
  * ``models``: per case the reference ``MM_FastVim`` (models/fastvim.py:560-691) in the configuration both mm* recipes
    use (``rms_norm=False, fused_add_norm=False, residual_in_fp32=True, final_pool_type="all", if_abs_pos_embed=True,
    rotate_every_block=True, drop_path_rate=0.0``), B = 2, training mode.  Parameters are ``oracle.make_state_dict(seed,
    shapes=<the model's own state-dict shapes>)`` and the image is ``randn`` of a seeded CPU generator: the fixture holds
    the RECIPE (kwargs, seeds, shapes, checksums of the image and of the seeded cotangents ``g_k``), not the weights.
    Stored in ``dense_<case>.pt``: the fp64 outputs and the fp64 gradients of ``sum_k <out_k, g_k>`` with respect to the
    image, ``pos_embed``, every ``outnorm_*`` parameter and the first / last block's ``norm.weight`` / ``norm.bias``.
    From a second run of the same model in fp32: the max-abs error of every fp32 output and gradient against its fp64
    value (``out_err_ref32``, ``err_ref32``: the reference's own rounding).
  * ``ln2d``: the reference ``LN2d`` class's state-dict key list and ``eps``, and per shape the recipe of the inputs
    (seed, checksums) with the fp64 gradients of the weight and the bias.
``dense_ln2d.pt``
  * per LN2d shape the reference class's fp64 output and input gradient as (positions, C) rows.  The output of the two
    largest maps -- (2, 256, 16, 16) alone is 1 MiB in fp64 -- is recorded at ``rows``: 32 seeded (n, h, w) positions
    (first and last included), all channels; the input gradient of maps above 10000 elements at 8 (``dx_rows``).

LN2d inputs are ``randn`` values rounded to bf16 (held in fp32), weights too are seeded: the same recorded output serves
the fp32 and the bf16 test of a shape.  Numbers, names and settings only, nothing of the reference's source.
"""
import importlib.util
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

from _ref_import import REF_ROOT, load_reference  # noqa: E402
from oracle import make_state_dict  # noqa: E402
from dense_recipe import LN2D_SHAPES, checksum, ln2d_inputs, seeded_randn  # noqa: E402  (tests/dense_recipe.py)

F64 = torch.float64

MM_KW = dict(patch_size=16, stride=16, rms_norm=False, fused_add_norm=False, residual_in_fp32=True, final_pool_type="all",
             if_abs_pos_embed=True, rotate_every_block=True, drop_path_rate=0.0)
MODEL_CASES = {
    "t_64x96": dict(img_size=(64, 96), embed_dim=192, depth=4, out_indices=[1, 3], seed=11, x_seed=101),
    "s_80x112": dict(img_size=(80, 112), embed_dim=384, depth=2, out_indices=[0, 1], seed=12, x_seed=102),
}
LN2D_Y_ROWS_ABOVE, LN2D_DX_ROWS_ABOVE = 40000, 10000      # elements: larger maps are recorded at 32 / 8 positions
BATCH = 2


def ln2d_rows(shape, seed, above, count):
    """Indices of the recorded (n, h, w) positions of a map with more than ``above`` elements (None = all of them)."""
    N, C, H, W = shape
    M = N * H * W
    if N * C * H * W <= above or M <= count:
        return None
    g = torch.Generator().manual_seed(seed * 10 + 9)
    rows = torch.randperm(M, generator=g)[:count - 2].tolist() + [0, M - 1]
    return torch.tensor(sorted(set(rows)), dtype=torch.long)


def grad_names(depth, n_out):
    names = ["pos_embed"]
    for i in range(n_out):
        names += [f"outnorm_{i}.weight", f"outnorm_{i}.bias"]
    for l in sorted({0, depth - 1}):
        names += [f"layers.{l}.norm.weight", f"layers.{l}.norm.bias"]
    return names


def record_model(ns, name, case):
    kw = dict(MM_KW, img_size=case["img_size"], embed_dim=case["embed_dim"], depth=case["depth"],
              out_indices=list(case["out_indices"]))
    model = ns.fastvim.MM_FastVim(**kw)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = make_state_dict(case["seed"], shapes=shapes)
    Hh, Ww = case["img_size"]
    x = seeded_randn(case["x_seed"], BATCH, 3, Hh, Ww)
    gh, gw = Hh // 16, Ww // 16
    g = [seeded_randn(case["x_seed"] * 10 + k, BATCH, case["embed_dim"], gh, gw) for k in range(len(case["out_indices"]))]
    names = grad_names(case["depth"], len(case["out_indices"]))
    runs = {}
    for dt in (F64, torch.float32):
        model.load_state_dict(sd, strict=True)
        m = model.to(dt).train()
        xi = x.to(dt).requires_grad_()
        outs = m(xi)
        outs = [outs] if torch.is_tensor(outs) else list(outs)
        loss = sum((o * gk.to(dt)).sum() for o, gk in zip(outs, g))
        m.zero_grad(set_to_none=True)
        loss.backward()
        params = dict(m.named_parameters())
        grads = {"x": xi.grad.detach().clone()}
        grads.update({n: params[n].grad.detach().clone() for n in names})
        runs[dt] = ([o.detach().clone() for o in outs], grads)
    outs64, grads64 = runs[F64]
    outs32, grads32 = runs[torch.float32]
    err32 = {n: float((grads32[n].double() - grads64[n]).abs().max()) for n in grads64}
    out_err32 = [float((a.double() - b).abs().max()) for a, b in zip(outs32, outs64)]
    print(f"{name}: outs {[tuple(o.shape) for o in outs64]} max|out| {[float(o.abs().max()) for o in outs64]} "
          f"fp32 out err {out_err32}")
    for n in grads64:
        print(f"  grad {n}: max {float(grads64[n].abs().max()):.4g} err_ref32 {err32[n]:.3g}")
    return {"model_kwargs": kw, "seed": case["seed"], "x_seed": case["x_seed"], "batch": BATCH, "shapes": shapes,
            "x_checksum": checksum(x), "g_checksums": [checksum(t) for t in g], "outs": outs64, "out_err_ref32": out_err32,
            "grads": grads64, "err_ref32": err32, "grad_names": ["x"] + names}


def load_ref_ln2d():
    """The reference LN2d class: detection/vitdet/simple_fpn.py executed with stubs for the mm* imports it does not need
    for that class."""
    class _Any:
        pass

    for mod, attrs in (("mmcv", {}), ("mmcv.cnn", {"ConvModule": _Any, "build_norm_layer": None}),
                       ("mmdet.utils", {"MultiConfig": _Any, "OptConfigType": _Any}), ("mmengine", {}),
                       ("mmengine.model", {"BaseModule": torch.nn.Module})):
        m = types.ModuleType(mod)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[mod] = m
    spec = importlib.util.spec_from_file_location("_ref_simple_fpn", os.path.join(REF_ROOT, "detection", "vitdet", "simple_fpn.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.LN2d


def record_ln2d(LN2d):
    meta = {"state_dict_keys": list(LN2d(96).state_dict().keys()), "eps": LN2d(96).eps, "cases": {}}
    maps = {}
    for i, shape in enumerate(LN2D_SHAPES):
        seed = 500 + i
        x, dy, w, b = ln2d_inputs(shape, seed)
        N, C, H, W = shape
        m = LN2d(C).double()
        with torch.no_grad():
            m.weight.copy_(w)
            m.bias.copy_(b)
        xi = x.double().requires_grad_()
        y = m(xi)
        (y * dy.double()).sum().backward()
        rows = ln2d_rows(shape, seed, LN2D_Y_ROWS_ABOVE, 32)
        dx_rows = ln2d_rows(shape, seed, LN2D_DX_ROWS_ABOVE, 8)
        to_rows = lambda t: t.detach().permute(0, 2, 3, 1).reshape(N * H * W, C)
        yr, dxr = to_rows(y), to_rows(xi.grad)
        yr = yr if rows is None else yr[rows]
        dxr = dxr if dx_rows is None else dxr[dx_rows]
        meta["cases"][shape] = {"seed": seed, "x_checksum": checksum(x.detach()), "dy_checksum": checksum(dy), "rows": rows,
                                "dx_rows": dx_rows,
                                "dw": m.weight.grad.clone(), "db": m.bias.grad.clone()}
        maps[shape] = {"y_rows": yr.contiguous().clone(), "dx_rows": dxr.contiguous().clone()}
        print(f"ln2d {shape}: {yr.shape[0]} of {N * H * W} positions recorded, max|y| {float(y.abs().max()):.4g}")
    return meta, maps


if __name__ == "__main__":
    ns = load_reference()
    models = {name: record_model(ns, name, case) for name, case in MODEL_CASES.items()}
    # the big tensors of a model case (fp64 outputs and gradients) go to a file per case: dense_<case>.pt
    out = {"models": {}}
    files = {"dense_ln2d.pt": None}
    for name, rec in models.items():
        files[f"dense_{name}.pt"] = {"outs": rec.pop("outs"), "grads": rec.pop("grads")}
        rec["tensors_file"] = f"dense_{name}.pt"
        out["models"][name] = rec
    out["ln2d"], files["dense_ln2d.pt"] = record_ln2d(load_ref_ln2d())
    out["ln2d"]["maps_file"] = "dense_ln2d.pt"
    files["dense.pt"] = out
    for f, obj in files.items():
        torch.save(obj, os.path.join(HERE, f))
        size = os.path.getsize(os.path.join(HERE, f))
        print(f, size, "bytes")
        assert size <= 1 << 20, f"{f} is over the 1 MiB limit for a committed file"
