"""MAE pre-training at the FastVim-L / -H widths (embed 1024 / patch 16, embed 1280 / patch 14): depth-2 models against
the fp64 oracle, the un-pooled Vim baselines, and the captured pre-training step of ``mae_FastVim_huge_dec512d2b``.

Procedure and tolerances of tests/test_mae_gpu.py::test_mae_bf16_step_vs_oracle: mask equal, fp32 loss within 5e-5 and
prediction within 1e-4 of max(1, |ref|), gradients within 1e-3 of max(1e-3, max|ref|); bf16 autocast loss within 5e-2,
prediction within 8e-2."""
import pytest
import torch

pytestmark = pytest.mark.gpu
F64 = torch.float64


def _err(a, b):
    return (a.double().cpu() - b.double().cpu()).abs().max().item()


@pytest.mark.parametrize("embed_dim,patch", [(1024, 16), (1280, 14)])
def test_mae_lh_depth2_vs_oracle(embed_dim, patch):
    from fastvim_amd.models_mae import MaskedAutoencoderViM
    from oracle import mae_forward_oracle
    torch.manual_seed(3)
    m = MaskedAutoencoderViM(img_size=224, patch_size=patch, stride=patch, depth=2, embed_dim=embed_dim,
                             decoder_embed_dim=128, decoder_depth=1, rms_norm=True, residual_in_fp32=True,
                             fused_add_norm=True).cuda()
    L = (224 // patch) ** 2
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(4))
    noise = torch.rand(2, L, generator=torch.Generator().manual_seed(5))
    p = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
    lref, pref, mref = mae_forward_oracle(p, x, noise, patch_size=patch, depth=2, decoder_depth=1, compute_dtype=F64)
    lref.backward()
    loss, pred, mask = m(x.cuda(), noise=noise.cuda())
    assert torch.equal(mask.cpu().double(), mref)
    print(f"loss {loss.item()!r} ref {lref.item()!r}; pred err {_err(pred, pref):.3e} scale {pref.abs().max().item():.3e}")
    assert abs(loss.item() - lref.item()) <= 5e-5 * max(1.0, abs(lref.item()))
    assert _err(pred, pref) <= 1e-4 * max(1.0, pref.abs().max().item())
    loss.backward()
    worst = 0.0
    for n, q in m.named_parameters():
        if q.grad is None:
            assert not q.requires_grad, n
            continue
        e = _err(q.grad, p[n].grad)
        worst = max(worst, e / max(1e-3, p[n].grad.abs().max().item()))
        assert e <= 1e-3 * max(1e-3, p[n].grad.abs().max().item()), (n, e, p[n].grad.abs().max().item())
    print(f"worst gradient error / max(1e-3, max|ref|): {worst:.3e}")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        lb, pb, mb = m(x.cuda(), noise=noise.cuda())
    assert torch.equal(mb.cpu().double(), mref)
    print(f"bf16 loss {lb.item()!r}; pred err {_err(pb, pref):.3e}")
    assert abs(lb.item() - lref.item()) <= 5e-2 * max(1.0, abs(lref.item()))
    assert _err(pb, pref) <= 8e-2 * max(1.0, pref.abs().max().item())


@pytest.mark.parametrize("name", ["mae_vim_huge_dec512d2b", "mae_vim_large_dec512d2b"])
def test_unpooled_mae_baselines_run_and_repeat(name):
    """The un-pooled Vim MAE encoders (49 kept tokens + class token through mamba_simple.Mamba at d_inner 2560 / 2048):
    forward + backward finite under bf16 autocast, and a second run bit-identical."""
    from fastvim_amd import fastvim_mae
    torch.manual_seed(1)
    m = getattr(fastvim_mae, name)(img_size=224, depth=2).cuda().train()
    x = torch.randn(2, 3, 224, 224, device="cuda")

    def run():
        m.zero_grad(set_to_none=True)
        torch.manual_seed(2)                      # the masking noise is drawn on the device
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = m(x, mask_ratio=0.75)[0]
        loss.backward()
        return loss.detach().clone(), {n: q.grad.clone() for n, q in m.named_parameters() if q.grad is not None}

    l1, g1 = run()
    l2, g2 = run()
    assert torch.isfinite(l1) and all(torch.isfinite(v).all() for v in g1.values())
    assert len(g1) > 10 and torch.equal(l1, l2) and g1.keys() == g2.keys()
    assert all(torch.equal(g1[k], g2[k]) for k in g1)


def test_mae_huge_pretraining_step_graph_replay_equals_eager():
    """``mae_FastVim_huge_dec512d2b(img_size=224, depth=2)`` (patch 14, 256 tokens, 64 kept) on the flat training state
    with the fused AdamW + EMA, the whole step captured as the benchmark captures it; fixed masking noise, so nothing
    depends on the in-graph RNG (tests/test_mae_gpu.py, graph replay against eager).  2 warm-up steps + 3 replays equal 5
    eager steps bit for bit in loss, parameters and EMA; over 20 replays on the fixed batch the loss goes down.  The
    learning rate is the recipe's base rate 1.5e-4 unscaled: scaled by batch 4 / 256 the parameters would move less than
    a bf16 step of their shadow copies in 20 steps."""
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    from fastvim_amd.models_mae import mae_FastVim_huge_dec512d2b
    B = 4
    x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(1)).cuda()
    noise = torch.rand(B, 256, generator=torch.Generator().manual_seed(2)).cuda()

    def make():
        torch.manual_seed(1234)
        m = mae_FastVim_huge_dec512d2b(img_size=224, depth=2).cuda().train()
        flat = FlatTrainingState(m)
        nd = {n for n, p in m.named_parameters() if p.ndim <= 1 or n.endswith(".bias") or n in m.no_weight_decay()
              or getattr(p, "_no_weight_decay", False)}
        return m, flat, FlatAdamW(flat, m, lr=1.5e-4, betas=(0.9, 0.95), weight_decay=0.05, no_decay=nd, ema_decay=0.9999)

    def one_step(m, flat, opt):
        flat.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = m(x, noise=noise)[0]
        loss.backward()
        flat.finish_backward()
        opt.step()
        return loss.detach()

    m1, f1, o1 = make()
    eager = [one_step(m1, f1, o1).item() for _ in range(5)]
    p_eager, ema_eager = f1.param_flat.clone(), o1.ema.clone()
    f1.close()
    m2, f2, o2 = make()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm = [one_step(m2, f2, o2).item() for _ in range(2)]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lb = one_step(m2, f2, o2)
    rep = []
    for _ in range(3):
        g.replay()
        rep.append(lb.item())
    torch.cuda.synchronize()
    assert warm + rep == eager, (warm + rep, eager)
    assert torch.equal(f2.param_flat, p_eager) and torch.equal(o2.ema, ema_eager)
    for _ in range(17):
        g.replay()
        rep.append(lb.item())
    torch.cuda.synchronize()
    f2.close()
    assert all(l == l for l in rep) and rep[-1] < rep[0], rep
