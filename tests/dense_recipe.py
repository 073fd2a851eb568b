"""Input recipes shared by ``tests/golden/gen_dense.py`` (which records what the reference computes on them) and the
dense-prediction tests (which rebuild them from the recorded seeds and verify the recorded checksums).  Plain helpers, no
fixtures; nothing here imports ``fastvim_amd`` or the reference."""
import torch

LN2D_SHAPES = [(2, 96, 5, 7), (3, 256, 7, 7), (2, 256, 16, 16), (1, 192, 1, 1), (2, 40, 3, 5), (2, 1024, 2, 3), (2, 384, 9, 13)]


def seeded_randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def checksum(t):
    t = t.double()
    return [float(t.sum()), float(t.abs().sum())]


def ln2d_inputs(shape, seed):
    """Inputs of one LN2d case (shared with the tests through the recorded seed): bf16-representable fp32 values; the
    map sits about two standard deviations off zero with a per-image scale."""
    N, C, H, W = shape
    r = lambda s, *sh: seeded_randn(seed * 10 + s, *sh)
    x = (r(0, N, C, H, W) * (1 + torch.arange(N).float())[:, None, None, None] + 2.0).bfloat16().float()
    dy = r(1, N, C, H, W).bfloat16().float()
    w = (1 + 0.1 * r(2, C)).bfloat16().float()
    b = (0.1 * r(3, C)).bfloat16().float()
    return x, dy, w, b
