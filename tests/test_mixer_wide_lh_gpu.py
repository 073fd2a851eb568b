"""The fused mixer at the FastVim-L / -H widths (d_model 1024 / 1280: d_inner 2048 / 2560) against the fp64 oracle.

Pattern and tolerances of tests/test_mixer_gpu.py::test_mixer_wide_models_vs_oracle (fp32: 2e-5 of the output scale,
5e-5 for d hidden, 2e-4 for every parameter gradient, each relative to max(1, max|ref|)), of
test_mixer_max_pool_vs_oracle (1e-5 / 5e-5 / 2e-4) and of test_mixer_bf16_vs_fp64_oracle (2e-2 / 3e-2 / 4e-2).

The grids pick the launch forms of csrc/mixer_plan.h: (3, 14) and (2, 16) the whole-row conv + pool kernels (6 and 4
pooling rows: row groups of 4 are not filled), (3, 5) / (3, 7) the generic kernels on odd columns -- two channel slabs
in the adjoint, and at d_inner 2560 in the forward --, (2, 32) the cell walkers of the 448 px grid; the combine kernels
hold the whole row in one block (2560: 5 waves x 8 channels per lane)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
F64 = torch.float64


def _err(a, b):
    return (a.double().cpu() - b.double().cpu()).abs().max().item()


def _perturbed(m):
    with torch.no_grad():
        for n, p_ in m.named_parameters():
            if n in ("D", "D_b", "layernorm.weight") or n.endswith("bias"):
                p_.add_(0.1 * torch.randn_like(p_))
    return {k: v.detach().cpu() for k, v in m.state_dict().items()}


def _check(m, sd, h, g, grid, transposed, tols, okw, autocast=False):
    from oracle import fastvim_mixer_oracle
    ty, td, tw = tols
    rows, cols = grid
    Bsz, Ltok = h.shape[:2]
    perm = (lambda t: t.reshape(Bsz, rows, cols, -1).transpose(1, 2).reshape(Bsz, Ltok, -1)) if transposed else (lambda t: t)
    m.zero_grad(set_to_none=True)
    hg = perm(h).contiguous().cuda().requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        y = m(hg, transposed_grid=transposed)
    p = {k: v.clone().requires_grad_() for k, v in sd.items()}
    hc = h.clone().requires_grad_()
    yref = fastvim_mixer_oracle(p, hc, grid, compute_dtype=F64, out_dtype=F64, **okw)
    e = _err(y, perm(yref))
    print(f"out err {e:.3e} scale {yref.abs().max().item():.3e}")
    assert e <= ty * max(1.0, yref.abs().max().item()), e
    y.backward(perm(g).contiguous().cuda().to(y.dtype))
    yref.backward(g.double())
    e = _err(hg.grad, perm(hc.grad))
    print(f"dh err {e:.3e} scale {hc.grad.abs().max().item():.3e}")
    assert e <= td * max(1.0, hc.grad.abs().max().item()), e
    for n, q in m.named_parameters():
        e = _err(q.grad, p[n].grad)
        print(f"{n} err {e:.3e} scale {p[n].grad.abs().max().item():.3e}")
        assert e <= tw * max(1.0, p[n].grad.abs().max().item()), (transposed, n, e, p[n].grad.abs().max().item())


@pytest.mark.parametrize("grid", [(3, 14), (2, 16), (3, 5), (2, 32)])
@pytest.mark.parametrize("d_model", [1024, 1280])
def test_mixer_lh_widths_vs_oracle(d_model, grid):
    from fastvim_amd.mamba_simple_faster import Mamba
    torch.manual_seed(d_model + grid[1])
    m = Mamba(d_model, token_size=list(grid)).cuda()
    sd = _perturbed(m)
    Ltok = grid[0] * grid[1]
    h, g = torch.randn(2, Ltok, d_model), torch.randn(2, Ltok, d_model)
    for transposed in (False, True):
        _check(m, sd, h, g, grid, transposed, (2e-5, 5e-5, 2e-4), {})


@pytest.mark.parametrize("kw", [dict(scaling_factor=0.25), dict(use_norm_after_ssm=False)])
def test_mixer_h_width_options_vs_oracle(kw):
    from fastvim_amd.mamba_simple_faster import Mamba
    torch.manual_seed(7)
    grid = (2, 16)
    m = Mamba(1280, token_size=list(grid), **kw).cuda()
    sd = _perturbed(m)
    h, g = torch.randn(2, 32, 1280), torch.randn(2, 32, 1280)
    okw = dict(use_norm_after_ssm=kw.get("use_norm_after_ssm", True), scaling_factor=kw.get("scaling_factor", 1))
    for transposed in (False, True):
        _check(m, sd, h, g, grid, transposed, (2e-5, 5e-5, 2e-4), okw)


@pytest.mark.parametrize("d_model,grid", [(1024, (2, 16)), (1280, (3, 7))])
def test_mixer_lh_widths_max_pool_vs_oracle(d_model, grid):
    from fastvim_amd.mamba_simple_faster import Mamba
    torch.manual_seed(d_model)
    m = Mamba(d_model, token_size=list(grid), collapse_method="max").cuda()
    sd = _perturbed(m)
    Ltok = grid[0] * grid[1]
    h, g = torch.randn(2, Ltok, d_model), torch.randn(2, Ltok, d_model)
    for transposed in (False, True):
        _check(m, sd, h, g, grid, transposed, (1e-5, 5e-5, 2e-4), dict(collapse_method="max"))


@pytest.mark.parametrize("d_model,grid", [(1024, (3, 14)), (1280, (2, 16))])
def test_mixer_lh_widths_bf16_vs_fp64_oracle(d_model, grid):
    """bf16 storage + fp32 math under autocast against the fp64 oracle on the bf16-rounded input (the formulation of
    tests/test_mixer_gpu.py::test_mixer_bf16_vs_fp64_oracle).  These grids take the whole-row adjoint with the second
    pooled-gradient addend (the x_proj product stays a separate bf16 tensor)."""
    from fastvim_amd.mamba_simple_faster import Mamba
    torch.manual_seed(d_model)
    m = Mamba(d_model, token_size=list(grid)).cuda()
    sd = _perturbed(m)
    Ltok = grid[0] * grid[1]
    h = torch.randn(2, Ltok, d_model).bfloat16().float()
    g = torch.randn(2, Ltok, d_model).bfloat16().float()
    for transposed in (False, True):
        _check(m, sd, h, g, grid, transposed, (2e-2, 3e-2, 4e-2), {}, autocast=True)


def test_vim_mixer_l_width_vs_oracle():
    """The un-pooled Vim mixer at d_model 1024: the same conv kernels with one column (rows x 1 x tokens)."""
    from fastvim_amd.mamba_simple import Mamba
    from oracle import vim_mixer_oracle
    torch.manual_seed(10)
    m = Mamba(1024).cuda()
    sd = _perturbed(m)
    h, g = torch.randn(2, 10, 1024), torch.randn(2, 10, 1024)
    p = {k: v.clone().requires_grad_() for k, v in sd.items()}
    hc = h.clone().requires_grad_()
    yref = vim_mixer_oracle(p, hc, compute_dtype=F64, out_dtype=F64)
    yref.backward(g.double())
    hg = h.cuda().requires_grad_()
    y = m(hg)
    assert _err(y, yref) <= 2e-5 * max(1.0, yref.abs().max().item()), _err(y, yref)
    y.backward(g.cuda())
    assert _err(hg.grad, hc.grad) <= 5e-5 * max(1.0, hc.grad.abs().max().item())
    for n, q in m.named_parameters():
        e = _err(q.grad, p[n].grad)
        assert e <= 2e-4 * max(1.0, p[n].grad.abs().max().item()), (n, e, p[n].grad.abs().max().item())


@pytest.mark.parametrize("grid,dtype", [((3, 14), torch.float32), ((2, 16), torch.bfloat16), ((3, 5), torch.float32),
                                        ((3, 5), torch.bfloat16), ((2, 32), torch.float32)])
@pytest.mark.parametrize("d_in", [2048, 2560])
def test_channel_slab_forms_equal_the_one_slab_kernels_on_channel_halves(d_in, grid, dtype):
    """Twin of the new conv + pool forms.  The shipped library reads no environment variable, so no hook can force a
    slab form at a width the one-slab kernels serve; but the conv, the pooling and the D skip never mix channels, so
    the launch at d_inner 2048 / 2560 must equal, bit for bit, two launches at d_inner 1024 / 1280 on the channel
    halves -- widths the kernels served before (1280 as 10 waves of channel pairs, or 5 waves x 4).  Every data tensor
    (pooled conv output, skip, dx) is compared bitwise; the parameter gradients are sums over rows whose grouping per
    block may differ: 1e-6 relative."""
    from fastvim_amd import mixer_ops as M
    torch.manual_seed(d_in + grid[1])
    rows, cols = grid
    B, Ltok, half = 2, rows * cols, d_in // 2
    dev = "cuda"
    xz = torch.randn(B, Ltok, 2 * d_in, device=dev).to(dtype)
    cw, cwb = 0.5 * torch.randn(d_in, 4, device=dev), 0.5 * torch.randn(d_in, 4, device=dev)
    cb, cbb = 0.1 * torch.randn(d_in, device=dev), 0.1 * torch.randn(d_in, device=dev)
    D, Db = torch.randn(d_in, device=dev), torch.randn(d_in, device=dev)
    d_o = torch.randn(B, Ltok, d_in, device=dev).to(dtype)
    dxc = torch.randn(2, B, rows, d_in, device=dev)

    def run(xz_, cw_, cb_, cwb_, cbb_, D_, Db_, d_o_, dxc_):
        xc, skip = M.conv_pool_fwd(xz_, cw_, cb_, cwb_, cbb_, rows, cols, False, False, 0.25, D=D_, D_b=Db_)
        dxz = torch.zeros_like(xz_)
        pr = M.conv_pool_bwd(xz_, d_o_, dxc_, cw_, cb_, cwb_, cbb_, D_, Db_, dxz, rows, cols, False, False, 0.25)
        return xc, skip, dxz[..., :xz_.shape[-1] // 2].clone(), pr.clone()

    xc, skip, dx, pr = run(xz, cw, cb, cwb, cbb, D, Db, d_o, dxc)
    for s in range(2):
        c = slice(s * half, (s + 1) * half)
        xz_h = torch.cat([xz[..., c], xz[..., d_in:][..., c]], -1).contiguous()
        xc_h, skip_h, dx_h, pr_h = run(xz_h, cw[c].contiguous(), cb[c].contiguous(), cwb[c].contiguous(), cbb[c].contiguous(),
                                       D[c].contiguous(), Db[c].contiguous(), d_o[..., c].contiguous(), dxc[..., c].contiguous())
        assert torch.equal(xc[..., c], xc_h) and torch.equal(skip[..., c], skip_h)
        assert torch.equal(dx[..., c], dx_h)
        # partial row layout: [dw (d*4) | dw_b (d*4) | db | db_b | dD | dD_b]
        pr, pr_h = pr.flatten(), pr_h.flatten()
        for seg, (o, w) in enumerate([(0, 4), (4 * d_in, 4)] + [((8 + q) * d_in, 1) for q in range(4)]):
            oh = 0 if seg == 0 else (4 * half if seg == 1 else (8 + seg - 2) * half)
            a = pr[o + c.start * w: o + c.stop * w]
            b = pr_h[oh: oh + half * w]
            assert (a - b).abs().max().item() <= 1e-6 * max(1.0, b.abs().max().item()), (s, seg)
