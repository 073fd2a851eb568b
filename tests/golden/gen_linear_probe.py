"""Record what the reference's linear-probe recipe computes, for ``tests/test_linear_probe_cpu.py`` and
``tests/test_sgd_lars_gpu.py`` (build container only: it imports the reference by path).

    python tests/golden/gen_linear_probe.py

Writes ``linear_probe.pt`` next to this file:

* ``lars``: per weight decay (0 and 0.05) the reference ``LARS`` (mae/lars.py) run for 6 steps on one (10, 24) weight and
  one (10,) bias with fixed gradients, ``lr=0.1``, in fp64 and in fp32 -- inputs and the trajectories of the parameters
  and momentum buffers as tensors.  The weight starts at all zeros (step 0: the ``param_norm > 0`` branch is not taken)
  and the weight's gradient of step 3 is all zeros (with weight decay 0 the update norm is 0: the inner branch);
* ``probe``: the parameter names and ``requires_grad`` flags ``SupervisedModule.__init__`` (mae/linear_imagenet.py:39-53)
  leaves on a 2-layer FastVim, the head's ``state_dict`` keys, and the standard deviation of the re-drawn head weight.

Numbers and names only, nothing of the reference's source.  ``linear_imagenet.py`` imports Lightning and torchmetrics at
module level; neither is needed for what is recorded, so both are stubbed here."""
import importlib.util
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from _ref_import import REF_ROOT, load_reference  # noqa: E402


def _load(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF_ROOT, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def record_lars():
    ref = _load("_ref_lars", "mae", "lars.py")
    g = torch.Generator().manual_seed(20240607)
    steps = 6
    w0 = torch.zeros(10, 24)
    b0 = torch.randn(10, generator=g) * 0.1
    gw = torch.randn(steps, 10, 24, generator=g)
    gb = torch.randn(steps, 10, generator=g)
    gw[3].zero_()
    out = {"steps": steps, "lr": 0.1, "momentum": 0.9, "trust_coefficient": 0.001, "weight": w0, "bias": b0,
           "grad_weight": gw, "grad_bias": gb, "runs": {}}
    for wd in (0.0, 0.05):
        for dt, tag in ((torch.float64, "fp64"), (torch.float32, "fp32")):
            w = torch.nn.Parameter(w0.to(dt).clone())
            b = torch.nn.Parameter(b0.to(dt).clone())
            opt = ref.LARS([w, b], lr=0.1, weight_decay=wd)
            tw, tb, mw, mb = [], [], [], []
            for s in range(steps):
                w.grad = gw[s].to(dt).clone()
                b.grad = gb[s].to(dt).clone()
                opt.step()
                tw.append(w.detach().clone())
                tb.append(b.detach().clone())
                mw.append(opt.state[w]["mu"].clone())
                mb.append(opt.state[b]["mu"].clone())
            out["runs"][(wd, tag)] = {"weight": torch.stack(tw), "bias": torch.stack(tb), "mu_weight": torch.stack(mw),
                                      "mu_bias": torch.stack(mb)}
            print(f"lars wd={wd} {tag}: |w| after {steps} steps = {tw[-1].norm().item():.6g}")
    return out


def record_probe():
    ns = load_reference()
    import torch.nn as nn

    class LightningModule(nn.Module):
        def save_hyperparameters(self, *a, **k):
            pass

    pl = types.ModuleType("pytorch_lightning")
    pl.LightningModule = LightningModule
    sys.modules["pytorch_lightning"] = pl
    sys.modules["pytorch_lightning.core"] = types.ModuleType("pytorch_lightning.core")
    opt_mod = types.ModuleType("pytorch_lightning.core.optimizer")
    opt_mod.LightningOptimizer = object
    sys.modules["pytorch_lightning.core.optimizer"] = opt_mod
    sys.modules["torchmetrics"] = types.ModuleType("torchmetrics")
    fn = types.ModuleType("torchmetrics.functional")
    fn.accuracy = None
    sys.modules["torchmetrics.functional"] = fn
    ref = _load("_ref_linear_imagenet", "mae", "linear_imagenet.py")

    torch.manual_seed(0)
    kw = dict(img_size=64, depth=2, embed_dim=64, num_classes=1000, rms_norm=True, residual_in_fp32=True, fused_add_norm=True,
              final_pool_type="mean", if_abs_pos_embed=True)
    backbone = ns.fastvim.VisionMamba(**kw)
    module = ref.SupervisedModule(backbone, num_classes=1000, weight_decay=0.0, blr=0.1, batch_size=8)
    flags = [(n, bool(p.requires_grad)) for n, p in module.backbone.named_parameters()]
    head_keys = sorted(k for k in module.backbone.state_dict() if k.startswith("head."))
    std = float(module.backbone.head[1].weight.std())
    print(f"probe: {len(flags)} parameters, {sum(f for _, f in flags)} trainable, head keys {head_keys}, head std {std:.5f}")
    return {"model_kwargs": kw, "flags": flags, "head_keys": head_keys, "head_weight_std": std,
            "bn": {"eps": module.backbone.head[0].eps, "momentum": module.backbone.head[0].momentum,
                   "affine": module.backbone.head[0].affine}}


if __name__ == "__main__":
    out = {"lars": record_lars(), "probe": record_probe()}
    torch.save(out, os.path.join(HERE, "linear_probe.pt"))
