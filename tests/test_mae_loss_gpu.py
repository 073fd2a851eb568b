"""The fused MAE reconstruction loss (csrc/mae_loss.hip) against its fp64 restatement (tests/mae_loss_ref.py): both
kernels, every shape at which the addressing can go wrong, both pred dtypes, both image sources, four kinds of mask."""
import pytest
import torch

import mae_loss_ref as R

pytestmark = pytest.mark.gpu

# Tolerances.  Not chosen: MEASURED.  For each (patch, pred dtype), the error of the EXISTING eager fp32 composition
# (``MaskedAutoencoderViM.forward_loss`` and its autograd, on the GPU) against the fp64 restatement -- the relative error of
# the loss and max|dpred - ref| / max|ref| --, the largest over this file's shapes of that patch, both norm_pix settings and
# the four masks (a single case can be exact by luck, which would make the bound 0; the largest is the composition's error
# for that number format).  The kernel is allowed 4 x that (fast-math reciprocal square root, another summation order),
# and for bf16 dpred 2^-8 relative on top: one bf16 rounding.  Source: the "accuracy" section of
# profiles/mae_loss_bench.log (tools/bench_mae_loss.py), which lists every case and the kernel's own error next to it.
#            (patch, bf16): (loss, dpred) error of the eager composition
EAGER_ERR = {
    (16, False): (9.800e-08, 3.023e-07),
    (16, True): (1.167e-07, 3.266e-03),
    (14, False): (6.563e-08, 1.475e-07),
    (14, True): (8.740e-08, 2.934e-03),
    (8, False): (9.710e-08, 2.791e-07),
    (8, True): (8.048e-08, 3.245e-03),
}
# -> bounds (loss, dpred): 16 fp32 (3.92e-07, 1.21e-06), 16 bf16 (4.67e-07, 1.70e-02), 14 fp32 (2.63e-07, 5.90e-07),
#    14 bf16 (3.50e-07, 1.56e-02), 8 fp32 (3.88e-07, 1.12e-06), 8 bf16 (3.22e-07, 1.69e-02).  The kernels' own maxima in that
#    log: loss 6.98e-08 / 7.82e-08 / 6.56e-08 / 1.20e-07 / 8.29e-08 / 8.05e-08, dpred 1.85e-07 / 3.27e-03 / 1.56e-07 /
#    2.93e-03 / 1.84e-07 / 3.25e-03 in the same order.


def bounds(patch, bf16):
    el, ed = EAGER_ERR[(patch, bf16)]
    return 4.0 * el, 4.0 * ed + (2.0 ** -8 if bf16 else 0.0)


_DEV = {}


def _dev(patch, px, N):
    """The case's tensors on the GPU, uploaded once."""
    key = (patch, px, N)
    if key not in _DEV:
        c = R.make_case(patch, px, N)
        _DEV[key] = {k: v.cuda() for k, v in c.items()}
    return _DEV[key]


def _offset_view(t):
    """The same values as a contiguous view that starts ONE element into its storage."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() == buf.data_ptr() + t.element_size()
    return v


def run(patch, px, N, bf16, norm_pix, u8, mask, g=None, misalign=False, pred=None, img=None):
    """-> dict(loss, loss_rows, row_stats, dpred) from one forward + backward of the fused loss."""
    from fastvim_amd.losses import _MAELossFn, mae_reconstruction_loss_ok
    d = _dev(patch, px, N)
    if img is None:
        img = d["u8"] if u8 else d["f32"]
    table = d["table"] if u8 else None
    if pred is None:
        pred = d["pred"].bfloat16() if bf16 else d["pred"]
    pred = pred.clone()
    if misalign:
        img, pred = _offset_view(img), _offset_view(pred)
    pred.requires_grad_(True)
    mask = mask.cuda()
    assert mae_reconstruction_loss_ok(img, pred, mask, patch, table)
    loss, rows, stats = _MAELossFn.apply(pred, img, mask, table, patch, norm_pix)
    if g is None:
        loss.backward()
    else:
        loss.backward(gradient=torch.tensor(g, device="cuda"))
    assert pred.grad.dtype == pred.dtype and pred.grad.shape == pred.shape
    return {"loss": loss.detach(), "loss_rows": rows, "row_stats": stats, "dpred": pred.grad}


def check(out, ref, mask, patch, bf16, norm_pix):
    bl, bd = bounds(patch, bf16)
    el, ed = R.errors(out["loss"], out["dpred"], ref)
    print(f"patch {patch} {'bf16' if bf16 else 'fp32'}: loss err {el:.3e} (bound {bl:.3e}), dpred err {ed:.3e} (bound {bd:.3e})")
    assert torch.isfinite(out["loss"]).item() and torch.isfinite(out["dpred"].float()).all().item()
    assert el <= bl, (el, bl)
    assert ed <= bd, (ed, bd)
    on = mask.bool()
    rows = out["loss_rows"].double().cpu()
    # a row is a sum of D <= 768 non-negative fp32 terms, 12 per lane in sequence and a 6-level tree: at most ~20 roundings of
    # 2^-24 each on the sum, and a few more in every term (target, difference, square): 32 x 2^-24 relative
    assert (rows[on] - ref["loss_rows"][on]).abs().max().item() <= 32 * 2.0 ** -24 * ref["loss_rows"][on].abs().max().item()
    assert torch.equal(rows[~on], torch.zeros_like(rows[~on]))
    assert torch.equal(out["dpred"].cpu()[~on], torch.zeros_like(out["dpred"].cpu()[~on]))
    if norm_pix:
        st = out["row_stats"].double().cpu()
        assert (st[..., 0][on] - ref["mean"][on]).abs().max().item() <= 1e-6 * max(1.0, ref["mean"][on].abs().max().item())
        assert ((st[..., 1][on] - ref["rstd"][on]).abs() / ref["rstd"][on]).max().item() <= 1e-5


@pytest.mark.parametrize("mask_kind", R.MASKS)
@pytest.mark.parametrize("u8", [False, True], ids=["f32img", "u8img"])
@pytest.mark.parametrize("norm_pix", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("patch,px,N", R.SHAPES)
def test_kernels_against_fp64(patch, px, N, bf16, norm_pix, u8, mask_kind):
    ref, mask = R.reference(patch, px, N, bf16, norm_pix, mask_kind)
    check(run(patch, px, N, bf16, norm_pix, u8, mask), ref, mask, patch, bf16, norm_pix)


@pytest.mark.parametrize("u8", [False, True], ids=["f32img", "u8img"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("patch,px,N", [(16, 48, 3), (14, 28, 2), (8, 16, 2)])
def test_misaligned_bases(patch, px, N, bf16, u8):
    """img and pred one element into their storage: +4 B (fp32), +2 B (bf16), +1 B (uint8).  The uint8 kernel needs no
    alignment (it then loads single bytes), so the predicate keeps that case on the kernel; same values as aligned."""
    ref, mask = R.reference(patch, px, N, bf16, True, "ratio75")
    out = run(patch, px, N, bf16, True, u8, mask, misalign=True)
    check(out, ref, mask, patch, bf16, True)
    aligned = run(patch, px, N, bf16, True, u8, mask)
    for k in aligned:
        assert torch.equal(out[k], aligned[k]), k


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("norm_pix", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("u8", [False, True], ids=["f32img", "u8img"])
def test_constant_patches(u8, norm_pix, bf16):
    """An all-zero uint8 image / an fp32 image of one repeated value: the centred second moment is exactly 0 (a one-pass
    E[t^2] - mean^2 would go negative here), the loss finite and equal to the reference, dpred finite."""
    patch, px, N = 16, 48, 3
    d = _dev(patch, px, N)
    if u8:
        img = torch.zeros_like(d["u8"])
        img_ref = R.pixel_norm()(img.cpu())
    else:
        img = torch.full_like(d["f32"], 0.7310585975646973)
        img_ref = img.cpu()
    pred = R.make_case(patch, px, N)["pred"]
    pred = pred.bfloat16() if bf16 else pred
    mask = R.make_mask("ratio75", N, pred.shape[1])
    ref = R.mae_loss_ref(img_ref, pred, mask, patch, norm_pix)
    out = run(patch, px, N, bf16, norm_pix, u8, mask, img=img)
    check(out, ref, mask, patch, bf16, False)
    if norm_pix and not u8:               # (the zero uint8 image normalises to one value PER CHANNEL: three values a patch)
        on = mask.bool()
        st = out["row_stats"].cpu()
        assert torch.equal(st[..., 0][on], torch.full_like(st[..., 0][on], 0.7310585975646973))      # the mean is the value
        assert (st[..., 1][on] - 1000.0).abs().max().item() <= 1e-3                                  # rsqrt(0 + 1e-6)


@pytest.mark.parametrize("u8", [False, True], ids=["f32img", "u8img"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("patch,px,N", [(16, 48, 3), (14, 28, 2)])
def test_skipped_rows_are_not_read(patch, px, N, bf16, u8):
    """pred rows of kept patches hold NaN: loss, loss_rows and dpred are what they are without the poison."""
    ref, mask = R.reference(patch, px, N, bf16, True, "ratio75")
    d = _dev(patch, px, N)
    pred = (d["pred"].bfloat16() if bf16 else d["pred"]).clone()
    pred[~mask.bool().cuda()] = float("nan")
    out = run(patch, px, N, bf16, True, u8, mask, pred=pred)
    clean = run(patch, px, N, bf16, True, u8, mask)
    for k in clean:
        assert torch.equal(out[k], clean[k]), k
    assert torch.equal(out["loss_rows"][~mask.bool().cuda()], torch.zeros_like(out["loss_rows"][~mask.bool().cuda()]))
    assert torch.equal(out["dpred"][~mask.bool().cuda()], torch.zeros_like(out["dpred"][~mask.bool().cuda()]))
    check(out, ref, mask, patch, bf16, True)


@pytest.mark.parametrize("mask_kind", ["ratio75", "one"])
@pytest.mark.parametrize("norm_pix", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("patch,px,N", R.SHAPES)
def test_uint8_equals_float_of_lookup_bit_for_bit(patch, px, N, bf16, norm_pix, mask_kind):
    from fastvim_amd.pixels import lookup
    d = _dev(patch, px, N)
    assert torch.equal(lookup(d["table"], d["u8"]), d["f32"])
    mask = R.make_mask(mask_kind, N, d["pred"].shape[1])
    a = run(patch, px, N, bf16, norm_pix, True, mask)
    b = run(patch, px, N, bf16, norm_pix, False, mask)
    for k in ("loss", "loss_rows", "row_stats", "dpred"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("u8", [False, True], ids=["f32img", "u8img"])
@pytest.mark.parametrize("patch,px,N", [(16, 48, 3), (14, 448, 1)])
def test_two_runs_are_bit_identical(patch, px, N, u8):
    mask = R.make_mask("ratio75", N, (px // patch) ** 2)
    a = run(patch, px, N, True, True, u8, mask)
    b = run(patch, px, N, True, True, u8, mask)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_upstream_gradient_of_one_half_halves_dpred_exactly(bf16):
    patch, px, N = 14, 28, 2
    mask = R.make_mask("ratio75", N, 4)
    one = run(patch, px, N, bf16, True, True, mask)
    half = run(patch, px, N, bf16, True, True, mask, g=0.5)
    assert torch.equal(half["dpred"].float(), one["dpred"].float() * 0.5)
    assert torch.equal(half["loss"], one["loss"])


def test_public_function_under_autocast_and_rows():
    """``mae_reconstruction_loss`` as the model calls it: a bf16 pred produced inside autocast, the loss fp32, the gradient
    back in the fp32 leaf; ``return_rows`` gives the per-patch errors."""
    from fastvim_amd.losses import mae_reconstruction_loss
    patch, px, N = 16, 32, 2
    d = _dev(patch, px, N)
    ref, mask = R.reference(patch, px, N, True, True, "ratio75")
    w = d["pred"].clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        pred = w.bfloat16()
        loss, rows = mae_reconstruction_loss(d["u8"], pred, mask.cuda(), patch, True, d["table"], return_rows=True)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and rows.shape == mask.shape and not rows.requires_grad
    loss.backward()
    el, ed = R.errors(loss.detach(), w.grad, ref)
    bl, bd = bounds(patch, True)
    assert el <= bl and ed <= bd, (el, ed)
