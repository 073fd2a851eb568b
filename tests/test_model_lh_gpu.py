"""FastVim-L / -H widths at the model level: depth-2 models (one even and one rotated layer) against the fp64 oracle,
and the MAE fine-tuning step (layer-wise lr decay, gradient clipping, Mixup / CutMix, DropPath, scaling_factor 0.25:
mae/config/finetune_FastVimH.yaml) on the flat training state, graph replay against the eager step.  The full-depth
factories (336 M / 685 M parameters) are exercised by tools/bench_lh.py, not here."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
F64 = torch.float64

_COMMON = dict(rms_norm=True, residual_in_fp32=True, fused_add_norm=True, final_pool_type="mean", if_abs_pos_embed=True)


def _err(a, b):
    return (a.double().cpu() - b.double().cpu()).abs().max().item()


@pytest.mark.parametrize("embed_dim,patch,img", [(1280, 14, 224), (1024, 16, 64)])
def test_depth2_lh_model_vs_oracle(embed_dim, patch, img):
    """Logits and every gradient, fp32, with the tolerances tests/test_model_gpu.py uses for its tiny models (2e-5 of the
    logit scale, 2e-4 for the gradients, relative to max(1, max|ref|)).  224 / 14 is the 16 x 16 grid of FastVim-H."""
    from fastvim_amd.fastvim import VisionMamba
    from oracle import fastvim_forward_oracle, make_state_dict
    m = VisionMamba(embed_dim=embed_dim, depth=2, img_size=img, patch_size=patch, stride=patch, num_classes=10,
                    drop_path_rate=0.0, **_COMMON).cuda().eval()
    sd = make_state_dict(seed=5, embed_dim=embed_dim, depth=2, img_size=img, patch_size=patch, num_classes=10)
    m.load_state_dict(sd, strict=True)
    x = torch.randn(2, 3, img, img, generator=torch.Generator().manual_seed(3))
    g = torch.randn(2, 10, generator=torch.Generator().manual_seed(4))
    logits = m(x.cuda())
    sdc = {k: v.clone().requires_grad_() for k, v in sd.items()}
    ref = fastvim_forward_oracle(sdc, x, patch_size=patch, depth=2, compute_dtype=F64)
    assert _err(logits, ref) <= 2e-5 * max(1.0, ref.abs().max().item()), (_err(logits, ref), ref.abs().max().item())
    logits.backward(g.cuda())
    ref.backward(g.double())
    for k, p in m.named_parameters():
        gref = sdc[k].grad
        e = _err(p.grad, gref)
        assert e <= 2e-4 * max(1.0, gref.abs().max().item()), (k, e, gref.abs().max().item())


def test_h_width_finetune_step_graph_replay_equals_eager():
    """bf16 autocast, drop_path_rate 0.3, scaling_factor 0.25, layer decay 0.75, max_grad_norm 3.0, Mixup / CutMix with
    label smoothing, batch 4, inside SegmentedTrainStep: 2 warm-up + 3 steps.  Losses finite, the optimizer saw finite
    gradients, the run repeated from the same seeds is bitwise equal, and graph replay is bitwise equal to the eager step
    on an identically initialised copy."""
    from fastvim_amd.fastvim import VisionMamba
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    from fastvim_amd.lr_decay import param_groups_lrd
    from fastvim_amd.mixup import Mixup
    from fastvim_amd.pipeline import SegmentedTrainStep
    B, C = 4, 10
    torch.manual_seed(0)
    base = VisionMamba(embed_dim=1280, depth=2, img_size=224, patch_size=14, stride=14, num_classes=C,
                       drop_path_rate=0.3, scaling_factor=0.25, **_COMMON).cuda().train()
    gen = torch.Generator(device="cuda").manual_seed(11)
    batches = [(torch.randn(B, 3, 224, 224, device="cuda", generator=gen), torch.randint(0, C, (B,), device="cuda", generator=gen))
               for _ in range(3)]
    seq = [(0.3172, False, None), (0.71, True, (40, 150, 0, 97)), (0.9, False, None)]

    def run(use_graph):
        m = copy.deepcopy(base)
        flat = FlatTrainingState(m)
        groups = param_groups_lrd(m, 0.05, no_weight_decay_list=m.no_weight_decay(), layer_decay=0.75)
        opt = FlatAdamW(flat, m, lr=1e-3, param_groups=groups, max_grad_norm=3.0, ema_decay=0.999)
        mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=C)
        mix.set(0.5)
        x = torch.zeros(B, 3, 224, 224, device="cuda")
        y = torch.zeros(B, dtype=torch.int64, device="cuda")
        x.copy_(batches[0][0]); y.copy_(batches[0][1])
        torch.manual_seed(7)
        step = SegmentedTrainStep(m, flat, opt, mix.criterion(), x, y, n_segments=2, use_graph=use_graph, warmup=2, mixup=mix)
        assert step.use_graph is use_graph
        losses, stats = [], []
        for (xb, yb), (lam, cut, box) in zip(batches, seq):
            x.copy_(xb); y.copy_(yb)
            mix.set(lam, use_cutmix=cut, box=box)
            losses.append(step.step().item())
            stats.append(opt.last_stats())
        torch.cuda.synchronize()
        out = (losses, stats, flat.param_flat.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.ema.clone())
        flat.close()
        return out

    g1 = run(True)
    assert all(l == l and abs(l) < 1e4 for l in g1[0]), g1[0]
    assert all(s["finite"] for s in g1[1]) and g1[1][-1]["skipped_steps"] == 0
    assert len(set(g1[0])) == 3
    g2 = run(True)
    e1 = run(False)
    for other, what in ((g2, "repeated graph run"), (e1, "eager step")):
        assert other[0] == g1[0] and other[1] == g1[1], (what, other[0], g1[0])
        for a, b in zip(other[2:], g1[2:]):
            assert torch.equal(a, b), what
    assert torch.isfinite(g1[2]).all() and torch.isfinite(g1[5]).all()
