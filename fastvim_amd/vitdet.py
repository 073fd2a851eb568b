"""ViTDet pieces of the detection recipe (detection/vitdet/simple_fpn.py) on the HIP kernels.

``LN2d`` (simple_fpn.py:15-32) is the recipe's ``norm_cfg=dict(type="LN2d")``: the neck, the three bbox heads and the mask
head normalise their (N, C, H, W) maps over the channel dimension with it.  Same constructor, parameter names,
initialisation and attributes as the reference class, without the mmdet registry decorator; ``forward`` is one launch of
``fastvim_amd.dense_ops.ln2d_fn`` (forward) and one for the backward instead of eight eager elementwise / reduction ops.
"""
import torch
import torch.nn as nn

from .dense_ops import ln2d_fn


class LN2d(nn.Module):
    """Channel LayerNorm of (batch_size, channels, height, width) inputs."""

    def __init__(self, normalized_shape, eps=1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(normalized_shape))
        self.bias = nn.Parameter(torch.zeros(normalized_shape))
        self.eps = eps
        self.normalized_shape = (normalized_shape,)

    def forward(self, x):
        return ln2d_fn(x, self.weight, self.bias, self.eps)
