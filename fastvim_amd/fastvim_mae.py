"""Vim masked autoencoder -- the UN-POOLED MAE baseline with a middle class token: mirror of models/mae/fastvim_mae.py
(``MaskedAutoencoderViM`` :309-709, factories ``mae_vim_{base,large,huge}_dec512d2b`` :714-767; the model
mae/config/pretrain_VimB.yaml pre-trains).  Same constructor kwargs, ``state_dict`` keys (``cls_token``, ``pos_embed`` /
``decoder_pos_embed`` with a leading class slot) and initialisation order as the reference.

Encoder and decoder are plain Vim blocks on the un-pooled Vim mixer (fastvim_amd/vim.py, fastvim_amd/mamba_simple.py) --
the encoder over the kept tokens with the class token in their middle, the decoder over the full grid with the class
token appended -- on the same fused HIP kernels as the FastVim MAE (fastvim_amd/models_mae.py), whose host-side helpers
(patchify, masking with a ``noise`` hook, loss, final norm) it inherits.

``fused_tokens`` (or a ``sampler``, the opt-in of the graph-replayed ``fastvim_amd.mae_step.VimMAEPretrainStep``): the token
bookkeeping around the class token -- encoder input and decoder input -- is one launch each way on the step's ``TokenPlan``
(fastvim_amd/mae_tokens.py: ``encoder_tokens_cls``, ``decoder_tokens_cls``) instead of the torch chain; same values, with
``cls_token.grad`` and ``mask_token.grad`` up to their summation order.
"""
from functools import partial

import numpy as np
import torch
import torch.nn as nn

from . import mae_tokens
from .fastvim import _init_weights, trunc_normal_
from .layernorm import RMSNorm
from .mamba_simple_faster import linear_module
from .models_mae import MaskedAutoencoderViM as _FastVimMAE, get_2d_sincos_pos_embed as _sincos_grid
from .vim import PatchEmbed, create_block


def get_2d_sincos_pos_embed(embed_dim, grid_size, cls_token=False):
    """(grid_size**2 (+ 1), embed_dim); ``cls_token``: a zero row in front (fastvim_mae.py:25-40)."""
    pe = _sincos_grid(embed_dim, grid_size)
    if cls_token:
        pe = np.concatenate([np.zeros([1, embed_dim]), pe], axis=0)
    return pe


class MaskedAutoencoderViM(_FastVimMAE):
    def __init__(self, img_size=224, patch_size=16, stride=16, depth=24, embed_dim=192, decoder_embed_dim=512,
                 decoder_depth=8, norm_pix_loss=True, channels=3, ssm_cfg=None, drop_rate=0.0,
                 norm_epsilon: float = 1e-5, rms_norm: bool = False, initializer_cfg=None, fused_add_norm=False,
                 residual_in_fp32=False, device=None, dtype=None, init_layer_scale=None, use_norm_after_ssm=True,
                 embed_layer=PatchEmbed, fused_loss=False, fused_tokens=False, **kwargs):
        factory_kwargs = {"device": device, "dtype": dtype}
        nn.Module.__init__(self)          # (the FastVim MAE's constructor builds pooled mixers: not wanted here)
        self.fused_loss = bool(fused_loss)
        self.fused_tokens = bool(fused_tokens)
        self.residual_in_fp32 = residual_in_fp32
        self.fused_add_norm = fused_add_norm
        self.d_model = self.num_features = self.embed_dim = embed_dim
        self.patch_size = patch_size
        in_chans = channels
        # ---- encoder (:349-388)
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim,
                                      strict_img_size=False, dynamic_img_pad=True)
        num_patches = self.patch_embed.num_patches
        self.num_patches = num_patches
        self.token_size = self.patch_embed.grid_size
        self.cls_token = nn.Parameter(torch.zeros(1, 1, self.embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, embed_dim), requires_grad=False)   # fixed sin-cos
        blk = partial(create_block, ssm_cfg=ssm_cfg, norm_epsilon=norm_epsilon, rms_norm=rms_norm,
                      residual_in_fp32=residual_in_fp32, fused_add_norm=fused_add_norm,
                      use_norm_after_ssm=use_norm_after_ssm, init_layer_scale=init_layer_scale, **factory_kwargs)
        self.layers = nn.ModuleList([blk(embed_dim, layer_idx=i) for i in range(depth)])
        self.norm_f = (nn.LayerNorm if not rms_norm else RMSNorm)(embed_dim, eps=norm_epsilon, **factory_kwargs)
        # ---- decoder (:392-426)
        self.decoder_embed = nn.Linear(embed_dim, decoder_embed_dim, bias=True)
        self.mask_token = nn.Parameter(torch.zeros(1, 1, decoder_embed_dim))
        self.decoder_pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, decoder_embed_dim), requires_grad=False)
        self.decoder_blocks = nn.ModuleList([blk(decoder_embed_dim, layer_idx=i) for i in range(decoder_depth)])
        self.decoder_norm = (nn.LayerNorm if not rms_norm else RMSNorm)(decoder_embed_dim, eps=norm_epsilon,
                                                                        **factory_kwargs)
        self.decoder_pred = nn.Linear(decoder_embed_dim, patch_size ** 2 * in_chans, bias=True)
        self.norm_pix_loss = norm_pix_loss
        # ---- initialisation, in the reference's order (:431-472)
        g = int(num_patches ** 0.5)
        self.pos_embed.data.copy_(torch.from_numpy(get_2d_sincos_pos_embed(embed_dim, g, cls_token=True)).float().unsqueeze(0))
        self.decoder_pos_embed.data.copy_(
            torch.from_numpy(get_2d_sincos_pos_embed(decoder_embed_dim, g, cls_token=True)).float().unsqueeze(0))
        w = self.patch_embed.proj.weight.data
        torch.nn.init.xavier_uniform_(w.view([w.shape[0], -1]))          # like nn.Linear, not nn.Conv2d
        trunc_normal_(self.cls_token, std=0.02)
        trunc_normal_(self.mask_token, std=0.02)
        self.decoder_embed.apply(self._init_weights_decoder)
        self.decoder_norm.apply(self._init_weights_decoder)
        self.decoder_pred.apply(self._init_weights_decoder)
        icfg = initializer_cfg if initializer_cfg is not None else {}
        self.decoder_blocks.apply(partial(_init_weights, n_layer=decoder_depth, **icfg))
        self.apply(partial(_init_weights, n_layer=depth, **icfg))

    @torch.jit.ignore
    def no_weight_decay(self):
        return {"pos_embed", "cls_token", "dist_token"}

    # The class token sits in the middle of the kept tokens and the blocks take no plan: this model does not share the FastVim
    # MAE's loops, so it does not offer the segment protocol of fastvim_amd.mae_step.MAEPretrainStep (which names the
    # missing method in its TypeError).  Its own protocol, for fastvim_amd.mae_step.VimMAEPretrainStep, is the ``_cls`` trio
    # below.
    _embed_masked = _run_layers = _tail = None

    def _mask_with_cls(self, x, mask_ratio, noise=None, sampler=None):
        """Masking and the class token in the MIDDLE of the kept tokens (:590-607) -> (tokens (N, K + 1, D), mask,
        ids_restore, plan).  ``x``: the patch embedding with its position rows added.

        ``fused_tokens`` or a ``sampler``: the inherited ``_masking`` makes the step's ``TokenPlan`` (where its predicate
        holds) and ``mae_tokens.encoder_tokens_cls`` assembles the tokens from the un-gathered ``x`` in one launch; where
        that says no, the torch chain runs on the gathered tokens.  Neither: ``plan`` is None and the code is the
        reference's, line for line."""
        plan = None
        if self.fused_tokens or sampler is not None:
            kept, mask, ids_restore, _, plan = self._masking(x, mask_ratio, noise, sampler, gather=False)
            if plan is not None:
                if mae_tokens.encoder_tokens_cls_ok(x, self.cls_token, self.pos_embed, plan):
                    return mae_tokens.encoder_tokens_cls(x, self.cls_token, self.pos_embed, plan), mask, ids_restore, plan
                kept = mae_tokens.gather_tokens(x, plan.keep_index, plan.restore_index)
            x = kept
        else:
            x, mask, ids_restore, _ = self.random_masking(x, mask_ratio, noise, sampler)
        M = x.shape[1]
        cls_tokens = (self.cls_token + self.pos_embed[:, :1, :]).expand(x.shape[0], -1, -1).to(x.dtype)
        token_position = M // 2
        x = torch.cat((x[:, :token_position, :], cls_tokens, x[:, token_position:, :]), dim=1)
        return x, mask, ids_restore, plan

    def forward_encoder(self, x, mask_ratio, inference_params=None, noise=None, sampler=None):
        """:583-631: patch embedding + position (the class slot of ``pos_embed`` goes to the class token), masking, the
        class token in the MIDDLE of the kept tokens, Vim blocks, final norm."""
        return self._encode(x, mask_ratio, inference_params, noise=noise, sampler=sampler)[:3]

    def _encode(self, x, mask_ratio, inference_params=None, noise=None, sampler=None):
        """``forward_encoder`` plus the step's ``TokenPlan`` (or None) as a fourth value, for ``forward_decoder``."""
        x = self.patch_embed(x, self.pos_embed[:, 1:, :])
        x, mask, ids_restore, plan = self._mask_with_cls(x, mask_ratio, noise, sampler)
        residual = None
        hidden_states = x
        for layer in self.layers:
            hidden_states, residual = layer(hidden_states, residual, inference_params=inference_params)
        return self._final_norm(self.norm_f, hidden_states, residual), mask, ids_restore, plan

    # ---- the segment protocol of fastvim_amd.mae_step.VimMAEPretrainStep: the FastVim MAE's (_embed_masked / _run_layers /
    # _tail) under names of its own -- the blocks take no plan, the tokens carry the class token.
    def _embed_masked_cls(self, imgs, mask_ratio, sampler):
        """Patch embedding + masking + the class token -> (tokens (N, K + 1, D), plan).  The keyed plan must apply."""
        x = self.patch_embed(imgs, self.pos_embed[:, 1:, :])
        tokens, _, _, plan = self._mask_with_cls(x, mask_ratio, None, sampler)
        if plan is None:
            raise RuntimeError("MaskedAutoencoderViM._embed_masked_cls: the keyed masking plan does not take these tokens "
                               f"({tuple(x.shape)} {x.dtype}, grid {tuple(self.token_size)}); see mae_tokens.plan_shape_ok")
        return tokens, plan

    def _run_layers_cls(self, hidden_states, residual, lo, hi, plan):
        """Encoder blocks ``lo .. hi - 1``; plain Vim blocks, which do not read the plan."""
        for layer in self.layers[lo:hi]:
            hidden_states, residual = layer(hidden_states, residual, inference_params=None)
        return hidden_states, residual

    def _tail_cls(self, hidden_states, residual, imgs, plan):
        """``norm_f``, the decoder and the reconstruction loss -> (loss, pred)."""
        latent = self._final_norm(self.norm_f, hidden_states, residual)
        pred = self.forward_decoder(latent, plan.ids_restore, plan=plan)
        return self._loss(imgs, pred, plan.mask), pred

    def forward_decoder(self, x, ids_restore, inference_params=None, plan=None):
        """:633-691: mask tokens appended and unshuffled WITHOUT the class token, which is re-attached at the END of the
        sequence, carried through the decoder blocks and dropped from the prediction.  ``plan``: the ``TokenPlan`` that
        ``ids_restore`` came from -- the decoder's input is then assembled by ``mae_tokens.decoder_tokens_cls`` where it takes
        the tensors; None: the torch chain."""
        token_position = (x.shape[1] - 1) // 2
        x = linear_module(self.decoder_embed, x)
        if plan is not None and mae_tokens.decoder_tokens_cls_ok(x, self.mask_token, self.decoder_pos_embed, plan):
            x = mae_tokens.decoder_tokens_cls(x, self.mask_token, self.decoder_pos_embed, plan)
            n = x.shape[1] - 1
        else:
            mask_tokens = self.mask_token.repeat(x.shape[0], ids_restore.shape[1] + 1 - x.shape[1], 1).to(x.dtype)
            x_ = torch.cat([x[:, :token_position, :], x[:, token_position + 1:, :], mask_tokens], dim=1)      # no cls token
            x_ = torch.gather(x_, dim=1, index=ids_restore.unsqueeze(-1).repeat(1, 1, x.shape[2]))            # unshuffle
            x_ = x_ + self.decoder_pos_embed[:, 1:]
            cls_tokens = x[:, token_position:token_position + 1, :] + self.decoder_pos_embed[:, :1, :]
            n = x_.shape[1]
            x = torch.cat([x_, cls_tokens.to(x_.dtype)], dim=1)
        residual = None
        for layer in self.decoder_blocks:
            x, residual = layer(x, residual, inference_params=inference_params)
        x = self._final_norm(self.decoder_norm, x, residual)
        x = linear_module(self.decoder_pred, x)
        return x[:, :n, :]                                           # remove cls token


def _mae_vim(embed_dim, depth, patch_size, stride, kwargs):
    depth = kwargs.pop("depth", depth)      # a shallower copy of the same widths (tests, tools); the reference fixes it
    model = MaskedAutoencoderViM(patch_size=patch_size, stride=stride, embed_dim=embed_dim, depth=depth,
                                 decoder_embed_dim=512, decoder_depth=2, rms_norm=True, residual_in_fp32=True,
                                 fused_add_norm=True, **kwargs)
    model.default_cfg = {}
    return model


def mae_vim_base_dec512d2b(patch_size=16, stride=16, **kwargs):
    return _mae_vim(768, 24, patch_size, stride, kwargs)


def mae_vim_large_dec512d2b(patch_size=16, stride=16, **kwargs):
    return _mae_vim(1024, 48, patch_size, stride, kwargs)


def mae_vim_huge_dec512d2b(patch_size=16, stride=16, **kwargs):
    return _mae_vim(1280, 64, patch_size, stride, kwargs)
