"""BatchNorm1d kernels (csrc/bn1d.hip: fv_bn1d_stats / fv_bn1d_apply / fv_bn1d_bwd) against torch's own batch norm in
fp64 on the CPU, applied to the storage-rounded inputs with the same running buffers.

Tolerances (none of them comes from the kernels' own results):

* fp32 outputs and the fp32 running buffers: 4 x the max abs error of torch's fp32 CPU ``F.batch_norm`` against the fp64
  reference ON THE SAME INPUTS, measured inside each test (fixed summation orders differ, hence the factor).  Measured on
  the build host with the seeds below, for orientation (max |fp32 - fp64| of torch's CPU batch norm, training forward):
      normal inputs          B=2: 2.4e-05   B=37: 3.9e-07   B=512: 5.0e-07     (max over d = 64, 192, 200, 1280)
      mean 100 / std 0.01    B=2: 7.5e-03   B=37: 1.3e-03   B=512: 2.1e-03     (the mean's fp32 rounding, divided by std)
      running_mean / _var    normal 1.4e-07 / 1.4e-07, mean-100 2.1e-06 / 1.4e-07; after 5 calls (B=37, d=192) 2.7e-08 / 2.7e-07
      backward dx            B=37, d=192, training: 4.8e-07
* bf16 outputs: within one bf16 ulp of the fp64 value, ``|err| <= 2^-8 |ref| + 1e-6`` -- half an ulp of rounding plus the
  fp32 error, derived, not measured.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = 1e-6
KINDS = ("normal", "offset", "constant")


def _inputs(kind, B, d, dtype, seed=0):
    """CPU fp32 tensor holding the STORAGE-ROUNDED values of the test input."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + d)
    x = torch.randn(B, d, generator=g)
    if kind == "offset":                       # (b) a one-pass E[x^2] - E[x]^2 fails here: 100^2 * 2^-24 >> 0.01^2
        x = 100.0 + 0.01 * x
    elif kind == "constant":                   # (c) one constant column
        x[:, d // 3] = 1.7
    return x.to(dtype).float()


def _ref(x, rm, rv, training, dt):
    """torch's batch norm in ``dt`` on the CPU -> (y, running_mean, running_var) in ``dt``."""
    rm, rv = rm.to(dt).clone(), rv.to(dt).clone()
    y = F.batch_norm(x.to(dt), rm, rv, None, None, training, 0.1, EPS)
    return y, rm, rv


def _check(got, ref64, ref32, what, dtype=torch.float32):
    err = (got.double().cpu() - ref64).abs()
    if dtype == torch.bfloat16:
        bound = ref64.abs() * 2.0 ** -8 + 1e-6
        print(f"{what}: max err {err.max().item():.3e} (bf16 ulp rule)")
        assert bool((err <= bound).all()), (what, err.max().item(), (err - bound).max().item())
    else:
        base = (ref32.double() - ref64).abs().max().item()
        print(f"{what}: max err {err.max().item():.3e}, torch fp32 CPU {base:.3e}, allowed {4 * base:.3e}")
        assert err.max().item() <= 4 * base, (what, err.max().item(), base)


def _fresh(d, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(d, generator=g) * 0.5, torch.rand(d, generator=g) + 0.5


def _run(x, dtype, rm, rv, training=True):
    from fastvim_amd.linear_probe import bn1d_apply, bn1d_stats
    xg = x.to(dtype).cuda()
    rmg, rvg = rm.clone().cuda(), rv.clone().cuda()
    nbt = torch.zeros((), dtype=torch.int64, device="cuda")
    table = bn1d_stats(xg) if training else None
    y, mean, rstd = bn1d_apply(xg, table, rmg, rvg, nbt if training else None, EPS, 0.1, training)
    torch.cuda.synchronize()
    return y, rmg, rvg, nbt, table


# B = 512 is the largest batch whose rows stay in registers between the passes, 513 the first that re-reads them;
# d = 200 is no multiple of the 64-column strip.
SHAPES = [(B, d) for B in (2, 37, 512) for d in (64, 192, 200, 1280)] + [(513, 64), (513, 200)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,d", SHAPES)
def test_training_forward_and_running_statistics(B, d, dtype):
    rm, rv = _fresh(d)
    for kind in KINDS:
        if kind == "offset" and dtype != torch.float32:
            continue
        x = _inputs(kind, B, d, dtype)
        y, rmg, rvg, nbt, table = _run(x, dtype, rm, rv)
        y64, rm64, rv64 = _ref(x, rm, rv, True, torch.float64)
        y32, rm32, rv32 = _ref(x, rm, rv, True, torch.float32)
        tag = f"{kind} B={B} d={d}"
        assert y.dtype == dtype and int(nbt) == 1 and float(table[-1]) == B
        _check(y, y64, y32, tag + " xhat", dtype)
        _check(rmg, rm64, rm32, tag + " running_mean")
        _check(rvg, rv64, rv32, tag + " running_var")
        if kind == "constant":
            c = d // 3
            assert bool((y[:, c] == 0).all()), "the constant column's xhat must be exactly 0"
            assert float(table[d + c]) == 0.0 and float(rvg[c]) <= 0.9 * float(rv[c]) * (1 + 1e-6)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_module_five_calls_then_eval(dtype):
    """The module over 5 consecutive training calls (running buffers against fp64 by the 4 x rule, the counter exactly
    5, the constant column's running variance decaying towards 0), then eval mode: buffers bit-unchanged, output from
    the running statistics."""
    from fastvim_amd.linear_probe import ProbeBatchNorm1d
    B, d = 37, 192
    bn = ProbeBatchNorm1d(d, affine=False, eps=EPS).cuda().train()
    rm64, rv64 = torch.zeros(d, dtype=torch.float64), torch.ones(d, dtype=torch.float64)
    rm32, rv32 = torch.zeros(d), torch.ones(d)
    c, prev = d // 3, 1.0
    for call in range(5):
        x = _inputs("constant", B, d, dtype, seed=call)
        y = bn(x.to(dtype).cuda())
        y64 = F.batch_norm(x.double(), rm64, rv64, None, None, True, 0.1, EPS)
        y32 = F.batch_norm(x, rm32, rv32, None, None, True, 0.1, EPS)
        _check(y, y64, y32, f"call {call} xhat", dtype)
        now = float(bn.running_var[c])
        assert now < prev and now <= 0.9 ** (call + 1) * (1 + 1e-6)
        prev = now
    _check(bn.running_mean, rm64, rm32, "running_mean after 5 calls")
    _check(bn.running_var, rv64, rv32, "running_var after 5 calls")
    assert int(bn.num_batches_tracked) == 5
    bn.eval()
    before = (bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone())
    x = _inputs("normal", B, d, dtype, seed=9)
    y = bn(x.to(dtype).cuda())
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (bn.running_mean, bn.running_var, bn.num_batches_tracked)))
    rmc, rvc = bn.running_mean.cpu(), bn.running_var.cpu()
    y64, _, _ = _ref(x, rmc, rvc, False, torch.float64)
    y32, _, _ = _ref(x, rmc, rvc, False, torch.float32)
    _check(y, y64, y32, "eval xhat", dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("d", [192, 200])
def test_two_table_rows_merge_to_the_whole_batch(d, dtype):
    """Two ranks in one process: statistics of the two halves of a batch (20 and 17 rows), the rows stacked, apply with
    world = 2 over all 37 rows -- xhat and the running buffers match the fp64 reference over the whole batch."""
    from fastvim_amd.linear_probe import bn1d_apply, bn1d_stats
    rm, rv = _fresh(d)
    for kind in KINDS:
        if kind == "offset" and dtype != torch.float32:
            continue
        x = _inputs(kind, 37, d, dtype)
        xg = x.to(dtype).cuda()
        table = torch.stack([bn1d_stats(xg[:20]), bn1d_stats(xg[20:])])
        assert table[:, -1].tolist() == [20.0, 17.0]
        rmg, rvg = rm.clone().cuda(), rv.clone().cuda()
        nbt = torch.zeros((), dtype=torch.int64, device="cuda")
        y, _, _ = bn1d_apply(xg, table, rmg, rvg, nbt, EPS, 0.1, True)
        y64, rm64, rv64 = _ref(x, rm, rv, True, torch.float64)
        y32, rm32, rv32 = _ref(x, rm, rv, True, torch.float32)
        _check(y, y64, y32, f"{kind} d={d} merged xhat", dtype)
        _check(rmg, rm64, rm32, f"{kind} d={d} merged running_mean")
        _check(rvg, rv64, rv32, f"{kind} d={d} merged running_var")
        assert int(nbt) == 1


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_backward_against_fp64_autograd(dtype, training):
    from fastvim_amd.linear_probe import ProbeBatchNorm1d
    B, d = 37, 192
    x = _inputs("normal", B, d, dtype)
    dy = _inputs("normal", B, d, dtype, seed=5)
    bn = ProbeBatchNorm1d(d, affine=False, eps=EPS).cuda().train(training)
    rm, rv = _fresh(d)
    with torch.no_grad():
        bn.running_mean.copy_(rm)
        bn.running_var.copy_(rv)
    xg = x.to(dtype).cuda().requires_grad_()
    bn(xg).backward(dy.to(dtype).cuda())
    refs = []
    for dt in (torch.float64, torch.float32):
        xr = x.detach().clone().to(dt).requires_grad_()
        F.batch_norm(xr, rm.to(dt).clone(), rv.to(dt).clone(), None, None, training, 0.1, EPS).backward(dy.to(dt))
        refs.append(xr.grad)
    assert xg.grad.dtype == dtype
    _check(xg.grad, refs[0], refs[1], f"dx training={training}", dtype)


def test_two_runs_are_bit_identical_and_a_replayed_graph_advances_the_counter():
    from fastvim_amd.linear_probe import ProbeBatchNorm1d
    rm, rv = _fresh(1280)
    x = _inputs("normal", 512, 1280, torch.float32)
    a, b = _run(x, torch.float32, rm, rv), _run(x, torch.float32, rm, rv)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    bn = ProbeBatchNorm1d(192, affine=False, eps=EPS).cuda().train()
    xg = _inputs("normal", 37, 192, torch.bfloat16).to(torch.bfloat16).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        bn(xg)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = bn(xg)
    torch.cuda.synchronize()
    n0, rv0 = int(bn.num_batches_tracked), bn.running_var.clone()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert int(bn.num_batches_tracked) == n0 + 3 and not torch.equal(rv0, bn.running_var)
    assert torch.isfinite(y.float()).all()


def test_refused_inputs():
    from fastvim_amd.linear_probe import ProbeBatchNorm1d, bn1d_stats
    bn = ProbeBatchNorm1d(64, affine=False, eps=EPS).cuda().train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        bn(torch.randn(1, 64, device="cuda"))
    with pytest.raises(ValueError, match="batch, features"):
        bn(torch.randn(2, 64, 3, device="cuda"))
    with pytest.raises(RuntimeError, match="fp32 or bf16"):
        bn1d_stats(torch.randn(4, 64, device="cuda").half())
    with pytest.raises(NotImplementedError, match="across ranks"):
        x = torch.randn(4, 64, device="cuda", requires_grad=True)
        bn.normalize(x, torch.zeros(2, 129, device="cuda"))
    bn.eval()
    assert bn(torch.randn(1, 64, device="cuda")).shape == (1, 64)      # eval takes a batch of 1, as torch does
