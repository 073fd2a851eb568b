"""The MAE pre-training step (the reference's ``SSLModule.training_step`` under Lightning's ``accumulate_grad_batches``:
mae/mae_imagenet.py:17,68-94, mae/pretrain.py:43, ``accum_iter`` of mae/config/pretrain_FastVim{B,L,H}.yaml) as the chain of
HIP graphs that ``fastvim_amd.pipeline.SegmentedTrainStep`` is for supervised training:

    [zero the flat gradient]  replay(fwd) -> replay(bwd 0) -> ... -> replay(bwd K-1)                        micro-batches 0 .. A-2
                              replay(fwd) -> replay(bwd 0), launch(bucket 0) -> ... -> finish() -> replay(opt)   micro-batch A-1

ONE forward graph (patch embedding, the keyed masking plan and the masking gather, the encoder blocks, ``norm_f``, the
decoder, the reconstruction loss), K backward graphs of one run of encoder blocks each, the last run first -- graph 0 also
holds the decoder and the loss -- and one optimizer graph.  The flat gradient is laid out ``[mask_token, patch_embed |
layers.0 .. layers.n | norm_f, decoder_*]`` (fastvim_amd/flat.py), so the bucket backward finishes first holds the decoder
and the one it finishes last the patch embedding and ``mask_token``.

Accumulation over ``accum_iter`` micro-batches: every micro-batch seeds its backward with 1 and adds into the flat gradient,
which is zeroed once, in front of micro-batch 0 and outside the graphs; the gradient exchange is launched behind the
backward graphs of the LAST micro-batch only (Lightning's ``no_sync`` on the others); the optimizer graph reads the sums
with ``grad_scale = 1 / (accum_iter * world)``.

The masks come from a ``fastvim_amd.mae_tokens.MaskSampler``: the plan launch inside the forward graph reads the sampler's
key block when it RUNS, so the caller draws between micro-batches, like ``opt.set_lr``:

    x.copy_(imgs, non_blocking=True); sampler.sample(); loss = step.micro_step()
"""
import torch

from . import mae_tokens
from .graph_chain import ChainStep

_PROTOCOL = ("_embed_masked", "_run_layers", "_tail")


class MAEPretrainStep(ChainStep):
    """``model``: a ``fastvim_amd.models_mae.MaskedAutoencoderViM`` in training mode (``_embed_masked / _run_layers / _tail``;
    a model without them -- the un-pooled ``fastvim_amd.fastvim_mae`` class -- raises ``TypeError``).  ``x``: the static image
    buffer the graphs read, normalised float pixels or, after ``fastvim_amd.pixels.attach_pixel_norm``, the uint8 batch.
    ``model.fused_loss`` is respected as set.  ``micro_step()`` runs one micro-batch and returns its device loss tensor;
    ``optimizer_ran`` says whether that call closed a group of ``accum_iter`` and stepped the optimizer; ``mask`` is the
    micro-batch's (B, L) mask.

    Capture needs ``warmup`` eager steps first; the training state, both RNG streams and the sampler's counter are
    snapshotted before and put back after them, so constructing the step leaves everything as it found it and the first
    ``micro_step()`` is step 0 of the trajectory.  ``use_graph=False`` runs the same sequence eagerly."""

    # the model's three segment methods -- embed + mask, a run of encoder blocks, the tail -- and the class that has them
    _protocol = _PROTOCOL
    _model_class = "fastvim_amd.models_mae.MaskedAutoencoderViM"

    def __init__(self, model, flat, opt, x, sampler, mask_ratio=0.75, accum_iter=1, n_segments=3, amp_dtype=torch.bfloat16,
                 use_graph=True, warmup=2):
        for name in self._protocol:
            if not callable(getattr(model, name, None)):
                raise TypeError(f"{type(self).__name__}: {type(model).__module__}.{type(model).__name__} has no {name}() -- the "
                                f"step cuts the encoder of {self._model_class} into runs of blocks that share one masking plan")
        if int(accum_iter) < 1:
            raise ValueError(f"MAEPretrainStep: accum_iter must be at least 1, got {accum_iter}")
        if not model.training:
            raise ValueError("MAEPretrainStep: the model is in eval mode; call model.train() first")
        grid = tuple(int(v) for v in model.token_size)
        len_keep = int(grid[0] * grid[1] * (1 - mask_ratio))
        if x.dim() != 4 or not mae_tokens.plan_shape_ok(x.shape[0], grid, len_keep):
            raise ValueError(f"MAEPretrainStep: the masking plan does not serve batch {tuple(x.shape)}, token grid {grid}, "
                             f"len_keep {len_keep} (mae_tokens.plan_shape_ok: at most {mae_tokens.MAX_TOKENS} tokens, at "
                             f"least {mae_tokens.MIN_KEEP} kept)")
        self.model, self.sampler = model, sampler
        self.mask_ratio, self.accum_iter, self.amp_dtype = float(mask_ratio), int(accum_iter), amp_dtype
        sampler.block(x.device)                          # the key block exists before any capture
        super().__init__(flat, opt, x, n_segments, use_graph, accum_iter=self.accum_iter)
        self.mask = None
        self.optimizer_ran = False
        self._micro = 0                                  # position inside the group of accum_iter micro-batches
        if use_graph:
            self._capture(warmup)

    # ------------------------------------------------------------------ the pieces
    def _forward(self):
        embed_masked, run_layers, tail = (getattr(self.model, name) for name in self._protocol)
        with torch.autocast("cuda", dtype=self.amp_dtype, enabled=self.amp_dtype != torch.float32):
            h, plan = embed_masked(self.x, self.mask_ratio, self.sampler)
            h, res = self._run_cuts(lambda lo, hi, h, res: run_layers(h, res, lo, hi, plan), (h, None))
            loss, _ = tail(h, res, self.x, plan)      # (graph 0 of the backward chain also holds the decoder and the loss)
        self.mask = plan.mask
        return self._end_forward(loss)

    # ------------------------------------------------------------------ capture / run
    def _snapshot(self):
        return (*super()._snapshot(), self.sampler.last()[1])

    def _restore(self, snap):
        super()._restore(snap)
        self.sampler.set_counter(snap[4])

    def _warm_step(self):                    # a whole step: a group of one micro-batch
        self.flat.zero_grad()
        self._eager()

    def micro_step(self):
        """One micro-batch on what ``x`` holds, with the masks of the sampler's last ``sample()``: forward and backward into
        the flat gradient; the last of a group also exchanges the gradient and steps the optimizer.  Returns the (device)
        loss tensor of the micro-batch."""
        last = self._micro == self.accum_iter - 1
        if self._micro == 0:
            self.flat.zero_grad()
        if not self.use_graph:
            self.loss = self._eager(last)
        else:
            self._replay(last)
        self._micro = 0 if last else self._micro + 1
        self.optimizer_ran = last
        return self.loss

    # ------------------------------------------------------------------ resume
    def state_dict(self):
        """The position inside the group and, inside a group, the gradient accumulated so far.  With the sampler's, the
        optimizer's and the model's state a resumed run continues bit for bit."""
        return {"micro": self._micro, "accum_iter": self.accum_iter,
                "grad_flat": self.flat.grad_flat.detach().clone() if self._micro else None}

    def load_state_dict(self, state):
        if int(state["accum_iter"]) != self.accum_iter:
            raise ValueError(f"MAEPretrainStep.load_state_dict: saved with accum_iter {state['accum_iter']}, this step has "
                             f"{self.accum_iter}")
        micro = int(state["micro"])
        if not 0 <= micro < self.accum_iter or (micro and state.get("grad_flat") is None):
            raise ValueError(f"MAEPretrainStep.load_state_dict: position {micro} of {self.accum_iter} without its gradient")
        if micro:
            with torch.no_grad():
                self.flat.grad_flat.copy_(state["grad_flat"])
        self._micro = micro


class VimMAEPretrainStep(MAEPretrainStep):
    """The same step for the Vim MAE baseline, ``fastvim_amd.fastvim_mae.MaskedAutoencoderViM`` (the reference's
    mae/config/pretrain_Vim{B,L}.yaml): the un-pooled encoder with a class token in the middle of the kept tokens.  The model
    offers the segment methods under names of its own (``_embed_masked_cls / _run_layers_cls / _tail_cls``; a model without
    them -- the FastVim MAE -- raises ``TypeError``); everything else is ``MAEPretrainStep``: ``micro_step()``,
    ``optimizer_ran``, ``mask``, ``accum_iter``, ``n_segments``, ``use_graph``, ``state_dict`` / ``load_state_dict``, and a
    construction that leaves the training state, both RNG streams and the sampler's counter as it found them.

    The forward graph holds the patch embedding, the keyed plan, ``mae_tokens.encoder_tokens_cls`` (the tokens of width
    K + 1 every run of blocks then carries), the blocks, ``norm_f``, the decoder behind ``mae_tokens.decoder_tokens_cls`` and
    the loss.  ``x`` may be the uint8 batch after ``fastvim_amd.pixels.attach_pixel_norm``: the model's patch embedding is the
    FastVim one in row-major order (fastvim_amd/vim.py: ``PatchEmbed``), which the pixel table serves.

    Flat layout (fastvim_amd/flat.py): ``cls_token`` and ``mask_token`` are parameters of the model itself, so both lie in
    the unit IN FRONT of the block stack, with the patch embedding -- ``[cls_token, mask_token, patch_embed | layers.0 ..
    layers.n | norm_f, decoder_*]``.  ``mask_token.grad`` is complete after backward graph 0 (the decoder), ``cls_token.grad``
    only after the last one (the run that holds the embedding); the front unit belongs to the bucket ``make_exchange``
    launches last, behind that graph, so both are exchanged complete."""

    _protocol = tuple(name + "_cls" for name in _PROTOCOL)
    _model_class = "fastvim_amd.fastvim_mae.MaskedAutoencoderViM"
