"""``MM_FastVim`` in the configuration both mm* recipes use (``rms_norm=False, fused_add_norm=False,
residual_in_fp32=True, final_pool_type="all"``, width 192 / 384) against what the reference itself computed in fp64
(tests/golden/gen_dense.py), and the route its feature taps take."""
import pytest
import torch

import norm_checks as nc
from conftest import load_golden
from dense_recipe import checksum, seeded_randn
from oracle import make_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = ["t_64x96", "s_80x112"]


def _build(case):
    from fastvim_amd.fastvim import MM_FastVim
    m = MM_FastVim(**case["model_kwargs"])
    m.load_state_dict(make_state_dict(case["seed"], shapes=case["shapes"]), strict=True)
    return m.to(DEV).train()


def _inputs(case):
    kw = case["model_kwargs"]
    Hh, Ww = kw["img_size"]
    x = seeded_randn(case["x_seed"], case["batch"], 3, Hh, Ww)
    assert checksum(x) == pytest.approx(case["x_checksum"], rel=1e-12)
    g = [seeded_randn(case["x_seed"] * 10 + k, case["batch"], kw["embed_dim"], Hh // 16, Ww // 16)
         for k in range(len(kw["out_indices"]))]
    for gk, cs in zip(g, case["g_checksums"]):
        assert checksum(gk) == pytest.approx(cs, rel=1e-12)
    return x.to(DEV), [gk.to(DEV) for gk in g]


def torch_taps(m, hiddens, H, W):
    """The composition the taps replace: cast, ``nn.LayerNorm``, ``view``, ``permute``, ``contiguous``."""
    C = m.embed_dim
    outs = [getattr(m, f"outnorm_{i}")(o.float()) for i, o in enumerate(hiddens)]
    return [o.view(-1, H, W, C).permute(0, 3, 1, 2).contiguous() for o in outs]


def _grads(m, x, outs, g, names):
    m.zero_grad(set_to_none=True)
    x.grad = None
    sum((o * gk).sum() for o, gk in zip(outs, g)).backward()
    params = dict(m.named_parameters())
    return {n: (x.grad if n == "x" else params[n].grad).detach().double().cpu() for n in names}


@pytest.fixture(scope="module", params=CASES)
def run(request):
    """One model per golden case; forward / backward with the fused taps and with the torch composition, shared by the
    tests below (nothing modifies it)."""
    case = load_golden("dense.pt")["models"][request.param]
    gold = load_golden(case["tensors_file"])
    m = _build(case)
    x, g = _inputs(case)
    x.requires_grad_()
    outs = m(x)
    assert isinstance(outs, list) and len(outs) == len(case["model_kwargs"]["out_indices"])
    new = _grads(m, x, outs, g, case["grad_names"])
    hiddens, (H, W) = m.forward_features(x, out_indices=m.out_indices)
    outs_t = torch_taps(m, hiddens, H, W)
    old = _grads(m, x, outs_t, g, case["grad_names"])
    return dict(name=request.param, case=case, gold=gold, m=m, x=x, outs=[o.detach() for o in outs],
                outs_torch=[o.detach() for o in outs_t], hiddens=[h.detach() for h in hiddens], HW=(H, W), new=new, old=old)


def test_outputs_vs_reference_fp64(run):
    for k, (o, ref) in enumerate(zip(run["outs"], run["gold"]["outs"])):
        assert o.dtype == torch.float32 and o.shape == ref.shape and o.is_contiguous()
        err = (o.double().cpu() - ref).abs().max().item()
        bound = 5e-5 * max(1.0, ref.abs().max().item())
        print(f"{run['name']} out {k}: err {err:.3e} bound {bound:.3e} (reference fp32 {run['case']['out_err_ref32'][k]:.3e})")
        assert err <= bound, (run["name"], k, err, bound)


def test_taps_take_the_fused_route(run):
    """Bit-identical to ``tap_layer_norm_nchw`` on the hidden states ``forward_features`` collects: pins the route."""
    from fastvim_amd.dense_ops import tap_layer_norm_nchw
    m, (H, W) = run["m"], run["HW"]
    for i, (o, h) in enumerate(zip(run["outs"], run["hiddens"])):
        norm = getattr(m, f"outnorm_{i}")
        assert h.dtype == torch.float32
        assert torch.equal(o, tap_layer_norm_nchw(h, norm.weight, norm.bias, H, W, norm.eps)), i


def test_gradients_vs_reference_fp64(run):
    """err_new <= 2 * max(err_torch, err_ref32) for every recorded gradient: the fused taps are as close to the fp64
    reference as the torch composition of the same model or the reference's own fp32 run (the factor 2 allows for fp32
    sums taken in another order)."""
    bad = []
    for n in run["case"]["grad_names"]:
        ref = run["gold"]["grads"][n]
        e_new = (run["new"][n] - ref).abs().max().item()
        e_old = (run["old"][n] - ref).abs().max().item()
        e_ref = run["case"]["err_ref32"][n]
        print(f"{run['name']} grad {n}: err_new {e_new:.3e} err_torch {e_old:.3e} err_ref32 {e_ref:.3e} (max|ref| {ref.abs().max().item():.3g})")
        if not e_new <= 2 * max(e_old, e_ref):
            bad.append((n, e_new, e_old, e_ref))
    assert not bad, bad


@pytest.mark.parametrize("name", CASES)
def test_bf16_autocast_outputs(name):
    """bf16 autocast, outputs only: the fused tap on the bf16 hidden states against their fp64 LayerNorm and against the
    torch composition on the same hidden states, per row within ``norm_checks``' y bound."""
    case = load_golden("dense.pt")["models"][name]
    m = _build(case)
    x, _ = _inputs(case)
    C = m.embed_dim
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        outs = m(x)
        hiddens, (H, W) = m.forward_features(x, out_indices=m.out_indices)
        outs_t = torch_taps(m, hiddens, H, W)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C)
    for i, (o, ot, h) in enumerate(zip(outs, outs_t, hiddens)):
        assert h.dtype in (torch.bfloat16, torch.float32) and o.dtype == torch.float32 and ot.dtype == torch.float32
        norm = getattr(m, f"outnorm_{i}")
        ref = nc.reference(h.reshape(-1, C), norm.weight, norm.bias, None, None, norm.eps, False, None, None)
        print(f"{name} tap {i}: hidden {h.dtype}, max|fused - torch| {(o - ot).abs().max().item():.3e}")
        msg = nc.check_y(rows(o), ref, norm.bias)                                      # against the fp64 LayerNorm
        assert not msg, (name, i, "fused vs fp64", msg)
        msg = nc.check_y(rows(o), dict(ref, y=rows(ot).double()), norm.bias)           # against the torch composition
        assert not msg, (name, i, "fused vs torch", msg)


def test_width_32_keeps_the_torch_composition():
    """embed_dim=32 (the model of test_mm_fastvim_multiscale_features) does not change path."""
    from fastvim_amd.fastvim import MM_FastVim
    torch.manual_seed(3)
    m = MM_FastVim(img_size=(64, 96), depth=4, embed_dim=32, out_indices=[1, 3], fused_add_norm=True,
                   residual_in_fp32=True, drop_path_rate=0.0).to(DEV).eval()
    x = torch.randn(2, 3, 64, 96, device=DEV)
    with torch.no_grad():
        outs = m(x)
        hiddens, (H, W) = m.forward_features(x, out_indices=m.out_indices)
        want = torch_taps(m, hiddens, H, W)
    assert not m._fused_taps(hiddens)
    for o, w in zip(outs, want):
        assert torch.equal(o, w)
