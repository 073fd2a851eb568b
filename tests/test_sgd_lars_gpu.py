"""FlatSGD (csrc/sgd_lars.hip: fv_sgd_flat, fv_lars_sumsq_partials, fv_lars_flat) on the parameter set of
tests/golden/linear_probe.pt -- one (10, 24) weight, one (10,) bias, 6 fixed gradients, lr 0.1, momentum 0.9.

Tolerances: 4 x what the same update in fp32 torch on the CPU deviates from the fp64 reference, measured inside each test
(none comes from the kernels' results).  For orientation, measured on the build host:
    torch.optim.SGD fp32 vs the fp64 restatement, 6 steps, over the four (grad_scale, weight_decay) cases:
        weight 2.0e-07 .. 3.4e-07, bias 3.4e-08 .. 8.7e-08, momentum buffers 1.2e-07 .. 6.9e-07
    the golden's own fp32 LARS run vs its fp64 run: weight 1.7e-07 / 1.9e-07 (weight decay 0 / 0.05), bias 8.7e-08,
        momentum buffers 4.0e-07 .. 5.4e-07
    torch.norm fp32 vs fp64 over 1000 x 1280 elements: |p| 1.5e-05, |g + wd p| 1.7e-05 relative (the exact norms rounded
        to fp32 are 3e-08 off)
The fused AdamW (csrc/optim.hip) is not touched by this optimizer: its file is byte-identical to its parent's.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

LR, MOM = 0.1, 0.9


class _Params(torch.nn.Module):
    def __init__(self, weight, bias):
        super().__init__()
        self.weight = torch.nn.Parameter(weight.clone())
        self.bias = torch.nn.Parameter(bias.clone())


def _start(gold, random_weight):
    lars = gold["lars"]
    w0 = lars["weight"].clone()
    if random_weight:
        w0 = torch.randn(10, 24, generator=torch.Generator().manual_seed(11)) * 0.3
    return w0, lars["bias"].clone(), lars["grad_weight"], lars["grad_bias"]


def _drive(model, opt, flat, gw, gb, grad_scale, each_step=None):
    """6 steps on the flat state; returns the trajectories (parameters and momentum buffers after every step)."""
    traj = {"weight": [], "bias": [], "mu_weight": [], "mu_bias": []}
    for s in range(gw.shape[0]):
        with torch.no_grad():
            model.weight.grad.copy_(gw[s])
            model.bias.grad.copy_(gb[s])
        opt.step(grad_scale=grad_scale)
        torch.cuda.synchronize()
        mu = opt._named_slices(opt.momentum_buf)
        traj["weight"].append(model.weight.detach().cpu().clone())
        traj["bias"].append(model.bias.detach().cpu().clone())
        traj["mu_weight"].append(mu["weight"].cpu().clone())
        traj["mu_bias"].append(mu["bias"].cpu().clone())
        for n, p in (("weight", model.weight), ("bias", model.bias)):      # the bf16 shadow follows every step
            assert torch.equal(p._fv_shadow, p.detach().to(torch.bfloat16)), (s, n)
        if each_step is not None:
            each_step(s)
    return {k: torch.stack(v) for k, v in traj.items()}


def _compare(got, ref64, ref32, what):
    for k in ("weight", "bias", "mu_weight", "mu_bias"):
        err = (got[k].double() - ref64[k]).abs().max().item()
        base = (ref32[k].double() - ref64[k]).abs().max().item()
        print(f"{what} {k}: max err {err:.3e}, fp32 torch on the CPU {base:.3e}, allowed {4 * base:.3e}")
        assert err <= 4 * base, (what, k, err, base)


@pytest.mark.parametrize("weight_decay", [0.0, 0.05])
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_flat_sgd_follows_torch_sgd(golden, grad_scale, weight_decay):
    from fastvim_amd.flat import FlatSGD, FlatTrainingState
    w0, b0, gw, gb = _start(golden("linear_probe.pt"), random_weight=True)
    # fp64 restatement: g' = g * grad_scale + wd * p; buf = momentum * buf + g'; p -= lr * buf
    ref64 = {k: [] for k in ("weight", "bias", "mu_weight", "mu_bias")}
    p = {"weight": w0.double(), "bias": b0.double()}
    buf = {k: torch.zeros_like(v) for k, v in p.items()}
    for s in range(6):
        for k, g in (("weight", gw[s]), ("bias", gb[s])):
            gd = g.double() * grad_scale + weight_decay * p[k]
            buf[k] = MOM * buf[k] + gd
            p[k] = p[k] - LR * buf[k]
            ref64[k].append(p[k].clone())
            ref64["mu_" + k].append(buf[k].clone())
    ref64 = {k: torch.stack(v) for k, v in ref64.items()}
    # what fp32 torch.optim.SGD on the CPU does with the same inputs (the gradient pre-scaled: exact for 1 and 0.5)
    cw, cb = torch.nn.Parameter(w0.clone()), torch.nn.Parameter(b0.clone())
    sgd = torch.optim.SGD([cw, cb], lr=LR, momentum=MOM, weight_decay=weight_decay)
    ref32 = {k: [] for k in ref64}
    for s in range(6):
        cw.grad, cb.grad = gw[s] * grad_scale, gb[s] * grad_scale
        sgd.step()
        ref32["weight"].append(cw.detach().clone())
        ref32["bias"].append(cb.detach().clone())
        ref32["mu_weight"].append(sgd.state[cw]["momentum_buffer"].clone())
        ref32["mu_bias"].append(sgd.state[cb]["momentum_buffer"].clone())
    ref32 = {k: torch.stack(v) for k, v in ref32.items()}
    model = _Params(w0, b0).cuda()
    with FlatTrainingState(model) as flat:
        opt = FlatSGD(flat, model, lr=LR, momentum=MOM, weight_decay=weight_decay)
        got = _drive(model, opt, flat, gw.cuda(), gb.cuda(), grad_scale)
    _compare(got, ref64, ref32, f"sgd gs={grad_scale} wd={weight_decay}")


def test_flat_sgd_no_decay_and_set_lr(golden):
    """``no_decay`` switches the decay off per parameter, ``set_lr`` reaches the kernel through device memory."""
    from fastvim_amd.flat import FlatSGD, FlatTrainingState
    w0, b0, gw, gb = _start(golden("linear_probe.pt"), random_weight=True)
    model = _Params(w0, b0).cuda()
    with FlatTrainingState(model) as flat:
        opt = FlatSGD(flat, model, lr=LR, momentum=MOM, weight_decay=0.5, no_decay=("bias",))
        opt.set_lr(0.25)
        with torch.no_grad():
            model.weight.grad.copy_(gw[0])
            model.bias.grad.copy_(gb[0])
        opt.step()
        torch.cuda.synchronize()
        wb = (b0.double() - 0.25 * gb[0].double())
        ww = (w0.double() - 0.25 * (gw[0].double() + 0.5 * w0.double()))
        assert (model.bias.detach().cpu().double() - wb).abs().max() < 1e-6
        assert (model.weight.detach().cpu().double() - ww).abs().max() < 1e-6


@pytest.mark.parametrize("weight_decay", [0.0, 0.05])
def test_flat_lars_follows_the_reference_trajectory(golden, weight_decay):
    """The reference LARS run recorded in the golden, fp64; tolerance 4 x the golden's own fp32-vs-fp64 deviation.  Step 0
    starts from an all-zero weight and step 3 has an all-zero weight gradient: q = 1 on both (with weight decay 0.05
    step 3's update is 0.05 p, not 0, so there only step 0 takes the branch)."""
    from fastvim_amd.flat import FlatSGD, FlatTrainingState
    gold = golden("linear_probe.pt")
    w0, b0, gw, gb = _start(gold, random_weight=False)
    assert not w0.any() and not gw[3].any()
    ref64, ref32 = gold["lars"]["runs"][(weight_decay, "fp64")], gold["lars"]["runs"][(weight_decay, "fp32")]
    model = _Params(w0, b0).cuda()
    qs = []
    with FlatTrainingState(model) as flat:
        opt = FlatSGD(flat, model, lr=gold["lars"]["lr"], momentum=gold["lars"]["momentum"], weight_decay=weight_decay,
                      lars=True, trust_coefficient=gold["lars"]["trust_coefficient"])
        got = _drive(model, opt, flat, gw.cuda(), gb.cuda(), 1.0, each_step=lambda s: qs.append(opt.last_norms()))
    _compare(got, ref64, ref32, f"lars wd={weight_decay}")
    assert qs[0]["weight"] == (0.0, qs[0]["weight"][1], 1.0) and qs[0]["weight"][1] > 0        # |p| = 0 -> q = 1
    if weight_decay == 0.0:
        assert qs[3]["weight"][1] == 0.0 and qs[3]["weight"][2] == 1.0 and qs[3]["weight"][0] > 0      # |dp| = 0 -> q = 1
    assert all(q["bias"] == (0.0, 0.0, 1.0) for q in qs)                                            # ndim <= 1: no q
    assert 0 < qs[1]["weight"][2] < 1


def test_lars_norms_at_the_recipe_size():
    """A (1000, 1280) head weight plus its bias, one LARS step: the two norms the trust ratio is made of against fp64,
    within 4 x the relative error of a plain fp32 ``torch.norm`` over the same elements."""
    from fastvim_amd.flat import FlatSGD, FlatTrainingState
    g = torch.Generator().manual_seed(5)
    w0 = torch.randn(1000, 1280, generator=g) * 0.01
    b0 = torch.zeros(1000)
    gw = torch.randn(1000, 1280, generator=g) * 1e-3
    gb = torch.randn(1000, generator=g) * 1e-3
    wd, trust = 0.05, 0.001
    model = _Params(w0, b0).cuda()
    with FlatTrainingState(model) as flat:
        opt = FlatSGD(flat, model, lr=LR, momentum=MOM, weight_decay=wd, lars=True, trust_coefficient=trust)
        with torch.no_grad():
            model.weight.grad.copy_(gw)
            model.bias.grad.copy_(gb)
        opt.step()
        torch.cuda.synchronize()
        pn, un, q = opt.last_norms()["weight"]
        w1 = model.weight.detach().cpu()
    dp64 = gw.double() + wd * w0.double()
    pn64, un64 = w0.double().norm().item(), dp64.norm().item()
    pn32, un32 = torch.norm(w0).item(), torch.norm(gw.add(w0, alpha=wd)).item()
    for name, got, r64, r32 in (("|p|", pn, pn64, pn32), ("|dp|", un, un64, un32)):
        err, base = abs(got - r64) / r64, abs(r32 - r64) / r64
        print(f"{name}: {got!r} vs fp64 {r64!r}: rel err {err:.3e}, fp32 torch.norm {base:.3e}, allowed {4 * base:.3e}")
        assert err <= 4 * base, (name, err, base)
    q64 = trust * pn64 / un64
    assert abs(q - q64) / q64 < 1e-6
    w64 = w0.double() - LR * dp64 * q64
    assert (w1.double() - w64).abs().max().item() < 1e-8      # 0.01-sized weights: 1e-8 is ~10 fp32 ulps
