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
import warnings

import torch
import torch.distributed as dist

from . import mae_tokens
from .pipeline import restore_training_state, snapshot_training_state

_PROTOCOL = ("_embed_masked", "_run_layers", "_tail")


class MAEPretrainStep:
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
        self.model, self.flat, self.opt, self.x, self.sampler = model, flat, opt, x, sampler
        self.mask_ratio, self.accum_iter, self.amp_dtype = float(mask_ratio), int(accum_iter), amp_dtype
        sampler.block(x.device)                          # the key block exists before any capture
        self.exchange = flat.make_exchange(n_segments)
        self.runs = self.exchange.layers                 # (lo, hi) block ranges in BACKWARD order
        self.K = len(self.runs)
        self._gscale = 1.0 / (self.accum_iter * self.exchange.world_size)
        self.use_graph = use_graph
        self.loss = self.mask = None
        self.optimizer_ran = False
        self._micro = 0                                  # position inside the group of accum_iter micro-batches
        self._seed = torch.ones((), device=x.device, dtype=torch.float32)      # d loss / d loss, allocated once outside the graphs
        self._cuts = None
        self.graphs = None
        if use_graph:
            self._capture(warmup)

    # ------------------------------------------------------------------ the pieces
    def _forward(self):
        m = self.model
        embed_masked, run_layers, tail = (getattr(m, name) for name in self._protocol)
        cuts = []              # per run in FORWARD order: (inputs (leaves) or None, outputs)
        with torch.autocast("cuda", dtype=self.amp_dtype, enabled=self.amp_dtype != torch.float32):
            h, plan = embed_masked(self.x, self.mask_ratio, self.sampler)
            res = None
            for i, (lo, hi) in enumerate(self.runs[::-1]):
                if i > 0:          # cut: this run's inputs are leaves that alias the previous run's outputs
                    h, res = h.detach().requires_grad_(), res.detach().requires_grad_()
                    ins = (h, res)
                else:
                    ins = None
                h, res = run_layers(h, res, lo, hi, plan)
                cuts.append([ins, (h, res)])
            loss, _ = tail(h, res, self.x, plan)
        cuts[-1][1] = (loss,)
        self._cuts = cuts
        self.mask = plan.mask
        return loss.detach()

    def _backward(self, k):
        """Backward of run k (backward order: k = 0 is the decoder, the loss and the last run of encoder blocks)."""
        i = self.K - 1 - k                      # forward index
        outs = self._cuts[i][1]
        if k == 0:
            torch.autograd.backward(outs[0], self._seed if outs[0].dtype == self._seed.dtype else None)
        else:
            nxt = self._cuts[i + 1][0]
            torch.autograd.backward(list(outs), [t.grad for t in nxt])
        self.flat.finish_backward()             # this run's queued weight-gradient GEMMs and partial sums
        self._cuts[i][1] = None                 # free the run's autograd graph

    # ------------------------------------------------------------------ capture / run
    def _eager_micro(self, last):
        loss = self._forward()
        for k in range(self.K):
            self._backward(k)
            if last:
                self.exchange.launch(k)
        if last:
            self.exchange.finish(mean=False)     # sums: the optimizer kernel applies 1 / (accum_iter world) as it reads them
            self.opt.step(grad_scale=self._gscale)
        return loss

    def _capture(self, warmup):
        from . import graph_capture_safe
        if not graph_capture_safe():
            # known to replay some captured steps wrongly (non-finite after a few replays): do not capture at all
            warnings.warn("MAEPretrainStep: HIP was initialised before `import fastvim_amd` could switch graph packet capture "
                          "off (DEBUG_CLR_GRAPH_PACKET_CAPTURE=0): on ROCm 7.2 some captured training steps replay wrongly "
                          "(DESIGN.md section 5) -- running this step EAGERLY instead.  Import fastvim_amd first, or export "
                          "the variable, to get graph replay.", RuntimeWarning, stacklevel=3)
            self.use_graph = False
            return
        snap, counter = snapshot_training_state(self.flat, self.opt), self.sampler.last()[1]
        pool = torch.cuda.graph_pool_handle()
        # (a live process group's watchdog thread polls events: "thread_local" keeps that legal during capture, pipeline.py)
        mode = "thread_local" if (dist.is_available() and dist.is_initialized()) else "global"
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):              # whole steps: allocator, lazily built buffers, RCCL communicators
                self.flat.zero_grad()
                self._eager_micro(True)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        restore_training_state(snap)
        self.sampler.set_counter(counter)
        torch.cuda.synchronize()
        g_fwd = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_fwd, pool=pool, capture_error_mode=mode):
            self.loss = self._forward()
        g_bwd = []
        for k in range(self.K):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=pool, capture_error_mode=mode):
                self._backward(k)
            g_bwd.append(g)
        g_opt = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_opt, pool=pool, capture_error_mode=mode):
            self.opt.step(grad_scale=self._gscale)
        self.graphs = (g_fwd, g_bwd, g_opt)

    def micro_step(self):
        """One micro-batch on what ``x`` holds, with the masks of the sampler's last ``sample()``: forward and backward into
        the flat gradient; the last of a group also exchanges the gradient and steps the optimizer.  Returns the (device)
        loss tensor of the micro-batch."""
        last = self._micro == self.accum_iter - 1
        if self._micro == 0:
            self.flat.zero_grad()
        if not self.use_graph:
            self.loss = self._eager_micro(last)
        else:
            g_fwd, g_bwd, g_opt = self.graphs
            g_fwd.replay()
            for k in range(self.K):
                g_bwd[k].replay()
                if last:
                    self.exchange.launch(k)
            if last:
                self.exchange.finish(mean=False)
                g_opt.replay()
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
