"""The masked (MAE) and un-pooled (Vim) mixers at the FastVim-L / -H widths (d_model 1024 / 1280: d_inner 2048 / 2560).

Both launch the fused row kernels as a ``rows x 1 x t`` grid: one patch column, every token its own pooling group.  At
d_inner 2560 the combine kernels hold the row as 5 waves x 8 channels per lane (csrc/mixer_plan.h, combine_wide8), a
form built for tokens_per_patch 1; the un-pooled grid is the same memory as ``rows*t x 1 x 1`` and is launched as that.
The caller's own re-described launch is the bitwise yardstick of whatever ``rows x 1 x t`` launches.

Procedure and tolerances of tests/test_masked_gpu.py::test_masked_mixer_vs_oracle and
tests/test_mixer_wide_lh_gpu.py::test_vim_mixer_l_width_vs_oracle: fp32 2e-5 / 5e-5 / 2e-4 for output / d hidden /
parameter gradients relative to max(1, max|ref|), bf16 2e-2 / 3e-2 / 4e-2."""
import pytest
import torch

pytestmark = pytest.mark.gpu
F64 = torch.float64


def _err(a, b):
    return (a.double().cpu() - b.double().cpu()).abs().max().item()


def _perturb(m):
    with torch.no_grad():
        for n, p_ in m.named_parameters():
            if n in ("D", "D_b", "layernorm.weight") or n.endswith("bias"):
                p_.add_(0.1 * torch.randn_like(p_))
    return {k: v.detach().cpu() for k, v in m.state_dict().items()}


@pytest.mark.parametrize("d_model,grid,keep,dtype", [
    (1024, (14, 14), 49, torch.float32),         # 49 = 7 x 7: odd t, one token in flight
    (1024, (14, 14), 49, torch.bfloat16),
    (1280, (16, 16), 64, torch.float32),         # MAE-H at 224 px: 64 = 16 x 4
    (1280, (16, 16), 64, torch.bfloat16),
    (1280, (4, 4), 6, torch.float32),            # 6 = 2 x 3
    (1280, (6, 10), 15, torch.float32),          # 15 = 5 x 3; rows of the grid without a kept token
])
def test_masked_mixer_lh_vs_oracle(d_model, grid, keep, dtype):
    from fastvim_amd.mamba_simple_masked_faster import Mamba_masked
    from oracle import masked_mixer_oracle
    torch.manual_seed(keep + d_model)
    rows, cols = grid
    m = Mamba_masked(d_model, token_size=list(grid)).cuda()
    sd = _perturb(m)
    Bsz = 2
    ids = torch.stack([torch.randperm(rows * cols)[:keep].sort().values for _ in range(Bsz)])
    h = torch.randn(Bsz, keep, d_model)
    g = torch.randn(Bsz, keep, d_model)
    bf = dtype == torch.bfloat16
    if bf:
        h, g = h.bfloat16().float(), g.bfloat16().float()
    p = {k: v.clone().requires_grad_() for k, v in sd.items()}
    hc = h.clone().requires_grad_()
    yref = masked_mixer_oracle(p, hc, ids, grid, compute_dtype=F64, out_dtype=F64)
    yref.backward(g.double())
    hg = h.cuda().requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf):
        y = m(hg, ids.cuda())
    tol_y, tol_dh, tol_w = (2e-2, 3e-2, 4e-2) if bf else (2e-5, 5e-5, 2e-4)
    e = _err(y, yref)
    print(f"out err {e:.3e} scale {yref.abs().max().item():.3e}")
    assert e <= tol_y * max(1.0, yref.abs().max().item()), e
    y.backward(g.cuda().to(y.dtype))
    e = _err(hg.grad, hc.grad)
    print(f"dh err {e:.3e} scale {hc.grad.abs().max().item():.3e}")
    assert e <= tol_dh * max(1.0, hc.grad.abs().max().item()), e
    for n, q in m.named_parameters():
        e = _err(q.grad, p[n].grad)
        print(f"{n} err {e:.3e} scale {p[n].grad.abs().max().item():.3e}")
        assert e <= tol_w * max(1.0, p[n].grad.abs().max().item()), (n, e, p[n].grad.abs().max().item())
    # deterministic: same inputs, same bits
    m.zero_grad(set_to_none=True)
    hg2 = h.cuda().requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf):
        y2 = m(hg2, ids.cuda())
    y2.backward(g.cuda().to(y2.dtype))
    assert torch.equal(y, y2) and torch.equal(hg.grad, hg2.grad)


@pytest.mark.parametrize("L", [10, 7, 21])      # one row of even t; one row of odd t; three 8-token rows, three pad tokens
def test_vim_mixer_h_width_vs_oracle(L):
    from fastvim_amd.mamba_simple import Mamba
    from oracle import vim_mixer_oracle
    torch.manual_seed(10 + L)
    m = Mamba(1280).cuda()
    sd = _perturb(m)
    h, g = torch.randn(2, L, 1280), torch.randn(2, L, 1280)
    p = {k: v.clone().requires_grad_() for k, v in sd.items()}
    hc = h.clone().requires_grad_()
    yref = vim_mixer_oracle(p, hc, compute_dtype=F64, out_dtype=F64)
    yref.backward(g.double())
    hg = h.cuda().requires_grad_()
    y = m(hg)
    e = _err(y, yref)
    print(f"out err {e:.3e} scale {yref.abs().max().item():.3e}")
    assert e <= 2e-5 * max(1.0, yref.abs().max().item()), e
    y.backward(g.cuda())
    e = _err(hg.grad, hc.grad)
    print(f"dh err {e:.3e} scale {hc.grad.abs().max().item():.3e}")
    assert e <= 5e-5 * max(1.0, hc.grad.abs().max().item()), e
    for n, q in m.named_parameters():
        e = _err(q.grad, p[n].grad)
        print(f"{n} err {e:.3e} scale {p[n].grad.abs().max().item():.3e}")
        assert e <= 2e-4 * max(1.0, p[n].grad.abs().max().item()), (n, e, p[n].grad.abs().max().item())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("rows,t", [(7, 7), (16, 4), (8, 8)])
@pytest.mark.parametrize("d_in", [2560, 2048])      # 2048: control, both forms existed before
def test_unpooled_combine_equals_the_redescribed_launch_bitwise(d_in, rows, t, dtype):
    """``rows x 1 x t`` and ``rows*t x 1 x 1`` address the same memory (token i*t + c, yc row i*t + c), so the
    tokens_per_patch > 1 launch must reproduce the tokens_per_patch 1 kernels bit for bit in every per-token tensor
    (at 2048 two different instantiations are compared, at 2560 the library re-describes the grid itself).
    The LayerNorm weight / bias gradients are sums over differently sized blocks: both launches within 1e-5 of the fp64
    sum of the same fp32 addends."""
    from fastvim_amd import mixer_ops as M
    torch.manual_seed(d_in + rows)
    B, Ltok, dev = 2, rows * t, "cuda"
    xz = torch.randn(B, Ltok, 2 * d_in, device=dev).to(dtype)
    skip = torch.randn(B, Ltok, d_in, device=dev).to(dtype)
    yc = torch.randn(2, B, Ltok, d_in, device=dev)
    dg = torch.randn(B, Ltok, d_in, device=dev).to(dtype)
    ln_w, ln_b = 1 + 0.1 * torch.randn(d_in, device=dev), 0.1 * torch.randn(d_in, device=dev)

    def run(r, tpp):
        g, mean, rstd = M.combine_fwd(xz, skip, yc, ln_w, ln_b, 1e-5, r, 1, False, tpp=tpp)
        dxz = torch.zeros_like(xz)
        d_o, dyct, p1 = M.combine_bwd(dg, xz, skip, yc, ln_w, ln_b, mean, rstd, dxz, r, 1, False, tpp=tpp)
        return g, mean, rstd, dxz, d_o, dyct.reshape(B, Ltok, d_in), p1.clone()

    a, b = run(rows, t), run(Ltok, 1)
    for k, name in enumerate(("g", "mean", "rstd", "dxz", "d_o", "dyct")):
        assert torch.equal(a[k], b[k]), name
    # the addends of d ln_w / d ln_b, formed in fp32 as the kernel forms them, summed in fp64
    mean, rstd = a[1].view(B, Ltok, 1), a[2].view(B, Ltok, 1)
    z = xz[..., d_in:].float()
    xhat = (0.5 * ((yc[0] + yc[1]) + skip.float()) - mean) * rstd
    dh = dg.float() * (z * torch.sigmoid(z))
    ref = torch.stack([(dh * xhat).double().sum((0, 1)), dh.double().sum((0, 1))])
    for p1 in (a[6], b[6]):
        for k in range(2):
            assert _err(p1[k], ref[k]) <= 1e-5 * max(1.0, ref[k].abs().max().item()), (k, _err(p1[k], ref[k]))


@pytest.mark.parametrize("in_dt,out_dt", [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16),
                                          (torch.bfloat16, torch.float32)])
def test_rows_segment_sum_and_gather_h_width_vs_torch(in_dt, out_dt):
    """tests/test_masked_gpu.py::test_rows_segment_sum_and_gather_vs_torch at d_inner 2560, its tolerances."""
    from fastvim_amd import mixer_ops as M
    torch.manual_seed(0)
    B, Lk, rows, d = 2, 11, 5, 2560
    x = torch.randn(2, B, Lk, d, device="cuda").to(in_dt)
    idx = torch.randint(0, rows, (2, B, Lk), device="cuda", dtype=torch.int32)
    idx[0, 0, :] = 2                                   # a row that takes everything, rows that take nothing
    out = M.rows_segment_sum(x, idx, rows, 0.25, out_dtype=out_dt)
    ref = torch.zeros(2, B, rows, d, device="cuda", dtype=F64)
    ref.scatter_add_(2, idx.long()[..., None].expand(2, B, Lk, d), x.double())
    tol = 1e-6 if out_dt == torch.float32 and in_dt == torch.float32 else 2e-2
    assert _err(out, 0.25 * ref) <= tol * max(1.0, ref.abs().max().item())
    y = torch.randn(2, B, rows, d, device="cuda").to(in_dt)
    gat = M.rows_gather(y, idx, 0.5, out_dtype=out_dt)
    refg = 0.5 * torch.gather(y.double(), 2, idx.long()[..., None].expand(2, B, Lk, d))
    assert _err(gat, refg) <= (1e-6 if out_dt == torch.float32 and in_dt == torch.float32 else 2e-2) * 4
