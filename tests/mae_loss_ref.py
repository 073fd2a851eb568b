"""fp64 restatement of the MAE reconstruction loss, in plain torch on the CPU, and the seeded cases the loss tests and
tools/bench_mae_loss.py share.

    n, l          patch (gy, gx) of image n, l = gy gw + gx
    j             (py p + px) 3 + c                    ("nhwpqc")
    t[j]          img[n, c, gy p + py, gx p + px]
    norm_pix:     mean = sum t / D, var = sum (t - mean)^2 / (D - 1), target = (t - mean) / sqrt(var + 1e-6); else target = t
    row           sum_j (pred[n, l, j] - target[j])^2 / D
    loss          sum(row mask) / sum(mask)
    dpred         g mask 2 (pred - target) / (D sum(mask))
"""
import functools

import torch

F64 = torch.float64

#         (patch, image px, N): the smallest shapes at which the addressing can fail -- L = 4; L = 9 with N L no multiple of
#         the 4 patches of a workgroup; patch 14 (8-byte bf16 rows, 56-byte fp32 / 14-byte uint8 segments); L = 1024; patch 8
SHAPES = ((16, 32, 2), (16, 48, 3), (14, 28, 2), (14, 448, 1), (8, 16, 2))
MASKS = ("ratio75", "all", "none_next_to_all", "one")


def patch_targets(img, p):
    """(N, 3, H, W) -> (N, L, D) fp64 in the order above, by explicit indexing (no reshape / permute of the image)."""
    img = img.to(F64)
    N, C, H, W = img.shape
    assert C == 3 and H % p == 0 and W % p == 0
    gh, gw = H // p, W // p
    out = torch.empty(N, gh * gw, p * p * 3, dtype=F64)
    for gy in range(gh):
        for gx in range(gw):
            blk = img[:, :, gy * p:(gy + 1) * p, gx * p:(gx + 1) * p]          # (N, c, py, px)
            out[:, gy * gw + gx] = blk.permute(0, 2, 3, 1).reshape(N, -1)        # (py, px, c)
    return out


def mae_loss_ref(img, pred, mask, p, norm_pix, g=1.0):
    """-> dict of fp64 tensors: loss (0-dim), loss_rows (N, L), mean, rstd (N, L), dpred (N, L, D)."""
    t = patch_targets(img, p)
    pred, mask = pred.to(F64), mask.to(F64)
    D = t.shape[-1]
    if norm_pix:
        mean = t.sum(-1, keepdim=True) / D
        var = ((t - mean) ** 2).sum(-1, keepdim=True) / (D - 1)
        rstd = 1.0 / torch.sqrt(var + 1.0e-6)
    else:
        mean, rstd = torch.zeros_like(t[..., :1]), torch.ones_like(t[..., :1])
    target = (t - mean) * rstd
    rows = ((pred - target) ** 2).sum(-1) / D
    sm = mask.sum()
    return {"loss": (rows * mask).sum() / sm, "loss_rows": rows, "mean": mean[..., 0], "rstd": rstd[..., 0],
            "dpred": g * mask[..., None] * 2.0 * (pred - target) / (D * sm)}


def make_mask(kind, N, L, seed=0):
    """(N, L) fp32, 1 = removed."""
    g = torch.Generator().manual_seed(1000 + seed)
    m = torch.zeros(N, L)
    if kind == "ratio75":                   # per sample, as random_masking leaves it: int(L / 4) kept
        keep = int(L * 0.25)
        for n in range(N):
            m[n, torch.randperm(L, generator=g)[keep:]] = 1.0
    elif kind == "all":
        m[:] = 1.0
    elif kind == "none_next_to_all":        # sample 0 keeps everything, the others lose everything (N = 1: the two halves)
        if N > 1:
            m[1:] = 1.0
        else:
            m[0, L // 2:] = 1.0
    elif kind == "one":                     # exactly one removed patch in the whole batch
        m[N - 1, (L // 2 + 1) % L] = 1.0
    else:
        raise ValueError(kind)
    return m


def pixel_norm():
    from fastvim_amd.pixels import IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD, PixelNorm
    return PixelNorm(IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD)


@functools.lru_cache(maxsize=None)
def make_case(patch, px, N):
    """Seeded CPU inputs of one shape: a uint8 image with smooth structure, noise and one constant (saturated) patch, its
    normalised fp32 form (the table lookup, so that both image kinds hold the same values) and an fp32 prediction.
    Cached and shared: treat as read-only."""
    g = torch.Generator().manual_seed(17 * patch + px + N)
    yy, xx = torch.meshgrid(torch.arange(px, dtype=torch.float32), torch.arange(px, dtype=torch.float32), indexing="ij")
    base = 128 + 90 * torch.sin(yy / 7.0)[None, None] * torch.cos(xx / 5.0 + torch.arange(3.0)[None, :, None, None])
    u8 = (base + 40 * torch.randn(N, 3, px, px, generator=g)).clamp(0, 255).to(torch.uint8)
    u8[0, :, :patch, :patch] = 255
    pn = pixel_norm()
    L = (px // patch) ** 2
    return {"u8": u8.contiguous(), "f32": pn(u8).contiguous(), "table": pn.table("cpu"),
            "pred": torch.randn(N, L, 3 * patch * patch, generator=g)}


@functools.lru_cache(maxsize=None)
def reference(patch, px, N, bf16, norm_pix, mask_kind):
    """The fp64 result for one case (on the bf16-rounded prediction when ``bf16``); cached, read-only."""
    c = make_case(patch, px, N)
    pred = c["pred"].bfloat16() if bf16 else c["pred"]
    mask = make_mask(mask_kind, N, pred.shape[1])
    return mae_loss_ref(c["f32"], pred, mask, patch, norm_pix), mask


def eager_composition(img, pred, mask, p, norm_pix):
    """The torch composition of ``MaskedAutoencoderViM.forward_loss`` -- what the fused kernels replace -- on whatever device
    and dtype the arguments have; returns (loss, dpred)."""
    pred = pred.detach().requires_grad_(True)            # a new leaf over the same storage
    N = img.shape[0]
    h = img.shape[2] // p
    t = img.reshape(N, 3, h, p, h, p).permute(0, 2, 4, 3, 5, 1).reshape(N, h * h, p * p * 3)
    if norm_pix:
        mean = t.mean(dim=-1, keepdim=True)
        var = t.var(dim=-1, keepdim=True)
        t = (t - mean) / (var + 1.0e-6) ** 0.5
    loss = (((pred - t) ** 2).mean(dim=-1) * mask).sum() / mask.sum()
    loss.backward()
    return loss.detach(), pred.grad


def errors(loss, dpred, ref):
    """(relative loss error, max-abs dpred error over the max-abs reference) against the fp64 ``ref``."""
    el = abs(loss.double().item() - ref["loss"].item()) / abs(ref["loss"].item())
    ed = (dpred.double().cpu() - ref["dpred"]).abs().max().item() / ref["dpred"].abs().max().item()
    return el, ed
