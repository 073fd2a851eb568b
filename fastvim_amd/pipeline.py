"""The data-parallel training step as a chain of HIP graphs with the gradient exchange between them.

torch DDP (what the reference trains with, imagenet_classification/train.py:34-43) overlaps its bucketed all-reduce
with backward through autograd hooks.  Here the step is captured into HIP graphs, so the overlap is made explicit
(SURVEY.md section 8e): the block stack is cut into K runs of blocks; ONE graph holds the forward pass, K graphs hold
the backward pass of one run each (last run first), one graph holds the fused optimizer.  The flat gradient is laid
out block by block (fastvim_amd/flat.py), so the gradient of run k is one contiguous bucket: as soon as backward graph
k has been enqueued, bucket k's all-reduce is launched asynchronously (RCCL, on the process group's stream, ordered
behind graph k by an event) and runs under backward graphs k+1 .. K-1:

    replay(fwd) -> replay(bwd 0), launch(bucket 0) -> replay(bwd 1), launch(bucket 1) -> ... -> finish() -> replay(opt)

Only the last bucket (the first blocks + patch embedding) is exposed.  Cutting backward needs the activations at the
cuts to be graph leaves: each run's input (hidden, residual) is a detached view of the previous run's output, and
backward of run k is ``torch.autograd.backward(outputs_k, grads of run k+1's inputs)``.  With one rank nothing is
exchanged and the chain computes what the single-graph step computes: bit for bit with ``gemm.FILL = False``; with
the shipped default (``gemm.fill_splits`` re-cuts a segment's smaller weight-gradient groups into more K slices) the
same sums are taken in another order and the two agree to rounding (tests/test_pipeline_gpu.py asserts both).

How the chain is captured and in what order it runs -- the capture mode under a live process group (the watchdog thread), the
warm-up, the cuts, the backward of a run -- is fastvim_amd/graph_chain.py, shared with the MAE pre-training step.
"""
import contextlib
import inspect
import warnings

import torch

from . import pixels
from .graph_chain import ChainStep, restore_training_state, snapshot_training_state      # noqa: F401  (both re-exported)


class SegmentedTrainStep(ChainStep):
    """``model`` must expose ``_embed / _run_layers / _final / _head``: fastvim_amd.fastvim.VisionMamba, the channel models
    (FastChannelVim and its 2-D compress variant), and the two un-pooled baselines with a middle class token, whose
    ``fused_cls`` puts that token's bookkeeping on the HIP path: fastvim_amd.vim.VisionMamba (``mixup`` / ``erase`` / uint8
    batches as for FastVim, no ``hcs``) and fastvim_amd.models_channel_mamba.VisionMamba (ChannelVim: ``hcs`` and uint8
    batches as for FastChannelVim; the class position follows the channel count of the family).
    ``loss_fn(logits, target) -> scalar``.  ``x`` / ``target`` are the static input buffers the graphs read; copy
    new batches into them between steps.  ``x`` holds normalised float pixels, or -- after
    ``fastvim_amd.pixels.attach_pixel_norm(model, mean, std)`` -- the uint8 batch itself, normalised inside the patch unfold.

    ``mixup`` (a ``fastvim_amd.mixup.Mixup``, with ``loss_fn = mixup.criterion()`` and ``target`` the (B,) int64 labels):
    the batch is mixed inside the step with the parameters of the last ``mixup.sample()``, which the caller issues between
    steps like ``opt.set_lr``:  ``x.copy_(batch); labels.copy_(y); mixup.sample(); opt.set_lr(lr); step.step()``.

    ``erase`` (a ``fastvim_amd.erasing.RandomErasing``): random erasing inside the step, after the normalisation and before the
    mixing, with the boxes and the noise key of the last ``erase.sample()`` -- the caller's, between steps, like
    ``mixup.sample()``; the step never draws.  A uint8 ``x`` is erased inside the patch unfold where that kernel applies;
    otherwise, and for a float ``x``, one ``fv_random_erase`` launch writes the erased batch into a scratch buffer of the step
    (never into ``x``: a replay without a fresh copy erases the same pixels again, nothing accumulates).  Not with ``hcs``:
    the cell recipes do not erase.

    ``hcs`` (a ``fastvim_amd.hcs.ChannelSampler``, for the channel models: ``model._embed`` must take ``hcs=``): hierarchical
    channel sampling inside the step.  The caller draws between steps -- ``x.copy_(batch); target.copy_(y); hcs.sample();
    opt.set_lr(lr); step.step()`` -- and the step embeds the sampler's current subset: the indices are read from its device
    array when the kernels run, the COUNT fixes every shape downstream, so one family of forward / backward graphs is
    captured per count 1..num_channels (largest first, into one memory pool: only one family runs at a time) and
    ``step()`` replays the family of ``hcs.count``; the optimizer graph does not depend on the count and is shared.

    Capture needs ``warmup`` eager steps first (allocator, lazily built buffers, RCCL communicators).  They are real
    steps on whatever ``x`` / ``target`` hold, so the training state they touch -- parameters, bf16 shadow, Adam moments,
    EMA, step count, the CPU and GPU RNG streams -- is snapshotted before and put back after them: constructing the
    step object leaves the model, the optimizer and the DropPath stream exactly as it found them."""

    def __init__(self, model, flat, opt, loss_fn, x, target, n_segments=3, amp_dtype=torch.bfloat16, use_graph=True,
                 warmup=2, mixup=None, hcs=None, erase=None):
        if erase is not None and hcs is not None:
            raise ValueError("SegmentedTrainStep: erase= and hcs= do not combine (the channel recipes of the reference do not "
                             "erase, and the per-channel unfold has no erase form)")
        self.model, self.loss_fn, self.target, self.amp_dtype = model, loss_fn, target, amp_dtype
        # batch-mode Mixup / CutMix inside the step: the images are mixed on their way into the patch embedding by whatever
        # the Mixup's device block holds when the graph RUNS -- the caller calls mixup.sample() between steps, the step never
        # does -- and `target` is the (B,) int64 label buffer that mixup.criterion() turns into the soft target
        self.mixup, self._embed_takes_mix, self._x_mixed = mixup, False, None
        if mixup is not None:
            mixup._check_batch(x)
            mixup.bind(x)                                # image size for the boxes; the block exists before any capture
            self._embed_takes_mix = "mix" in inspect.signature(model._embed).parameters
            if not self._embed_takes_mix:                # such a model gets the mixed batch from one fv_mix_batch launch
                # (a uint8 `x` -- fastvim_amd/pixels.py -- is normalised by the eager table lookup first and mixed after it, in
                # fp32: the mixed batch is a float buffer, what the embed would have been handed by a host-side loader)
                self._x_mixed = torch.empty_like(x, memory_format=torch.contiguous_format,
                                                 dtype=torch.float32 if x.dtype == torch.uint8 else x.dtype)
        # random erasing inside the step: the boxes and the key of erase's device block when the graph RUNS.  Inside the
        # embedding (the uint8 unfold kernel) for a uint8 `x` and a model whose _embed takes `erase=`; else into `_x_erased`,
        # after the table lookup and in front of the mixing
        self.erase, self._embed_takes_erase, self._x_erased = erase, False, None
        if erase is not None:
            erase.bind(x)                                # batch and image size; the block exists before any capture
            self._embed_takes_erase = (x.dtype == torch.uint8 and "erase" in inspect.signature(model._embed).parameters
                                       and (mixup is None or self._embed_takes_mix))
            if not self._embed_takes_erase:
                self._x_erased = torch.empty_like(x, memory_format=torch.contiguous_format,
                                                  dtype=torch.float32 if x.dtype == torch.uint8 else x.dtype)
        # hierarchical channel sampling: the subset of the sampler's device array, one family of graphs per channel count
        self.hcs = hcs
        if hcs is not None and "hcs" not in inspect.signature(model._embed).parameters:
            raise TypeError("SegmentedTrainStep: hcs= needs a model whose _embed takes the sampler (`_embed(x, hcs=None)`: "
                            "the channel models fastvim_amd.models_channel_mamba_faster.VisionMamba, its 2-D compress variant and "
                            "fastvim_amd.models_channel_mamba.VisionMamba; fastvim.VisionMamba and vim.VisionMamba embed all "
                            "channels)")
        if hcs is not None:
            hcs.block(x.device)                          # the index array exists before any capture
        super().__init__(flat, opt, x, n_segments, use_graph)
        self._exposed = []                               # (event before finish, event after) of the timed steps
        self.families = None                             # with hcs: {count: (forward graph, backward graphs, loss tensor)}
        if use_graph:
            pe = getattr(model, "patch_embed", None)
            if hcs is None and model.training and getattr(pe, "hcs", False) is True:
                warnings.warn("SegmentedTrainStep: the model samples channels (patch_embed.hcs) and no hcs= sampler was given: "
                              "the subset drawn during capture is frozen into the graphs and every replay embeds it.  Pass "
                              "hcs=fastvim_amd.hcs.ChannelSampler(channels) and call its sample() between steps.",
                              RuntimeWarning, stacklevel=2)
            self._capture(warmup)

    # ------------------------------------------------------------------ the pieces
    def _forward(self):
        m = self.model
        self.flat.zero_grad()
        with torch.autocast("cuda", dtype=self.amp_dtype, enabled=self.amp_dtype != torch.float32):
            kw = {} if self.hcs is None else {"hcs": self.hcs}
            x = self.x
            if self._embed_takes_erase:
                kw["erase"] = self.erase
            elif self.erase is not None:      # normalise, then erase out of place: `x` from here on is the float scratch batch
                xin = pixels.normalise_like(m, x) if x.dtype == torch.uint8 else x
                x = self.erase.erase(xin, out=self._x_erased)
            if self.mixup is None:
                h, _ = m._embed(x, **kw)
            elif self._embed_takes_mix:
                h, _ = m._embed(x, mix=self.mixup, **kw)
            else:              # (the channel models: the whole image is mixed before channels are selected, the reference's order)
                xin = pixels.normalise_like(m, x) if x.dtype == torch.uint8 else x
                h, _ = m._embed(self.mixup.mix_batch(xin, out=self._x_mixed), **kw)
            open_runs = hasattr(m, "_run_layers_open")

            def run(lo, hi, a, res, w=None):
                # w: the chain of fused blocks continues across the cut (fastvim._run_layers_open) -- the weight of its
                # pending out_proj; `a`, the activation that crosses the cut, is then the gated one and not the hidden state
                if not open_runs:
                    return m._run_layers(a, res, lo, hi)
                h, res, pend = m._run_layers_open(a if w is None else None, res, lo, hi, pend=None if w is None else (a, w))
                return (h, res) if pend is None else (pend[0], res, pend[1])

            h, res, *w = self._run_cuts(run, (h, None))
            if w:
                h = m._close_run((h, w[0]))
            logits = m._head(m._final(h, res))
        return self._end_forward(self.loss_fn(logits, self.target))

    # ------------------------------------------------------------------ capture / run
    def _snapshot(self):
        return (*snapshot_training_state(self.flat, self.opt), None if self.hcs is None else self.hcs.last())

    def _restore(self, snap):
        restore_training_state(snap[:4])
        if snap[4] is not None:
            self.hcs.set(snap[4])

    def _capture_families(self, warmup, snap, pool, mode):
        own, snap = snap[4], (*snap[:4], None)           # (a family keeps the subset it was warmed up with for its capture)
        if self.hcs is None:
            return self._capture_family(warmup, snap, pool, mode)
        # one family per channel count, the largest first (it sizes the shared pool); each is warmed up and captured with
        # the first c channels in the array -- a replay reads whatever the array holds then
        self.families = {}
        for c in range(self.hcs.num_channels, 0, -1):
            self.hcs.set(range(c))
            self.families[c] = self._capture_family(warmup, snap, pool, mode)
        self.hcs.set(own)                                # the sampler's own selection again
        return self.families[self.hcs.count]

    @contextlib.contextmanager
    def _time_exposed(self):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        yield
        e1.record()
        self._exposed.append((e0, e1))

    def step(self, time_exposed=False):
        """One training step; returns the (device) loss tensor.  ``time_exposed`` brackets the wait for the gradient
        exchange with events (read them with ``exposed_ms()`` after a synchronize)."""
        if not self.use_graph:
            self.loss = self._eager()
            return self.loss
        if self.families is not None:                    # the family of the sampler's current count
            g_fwd, g_bwd, self.loss = self.families[self.hcs.count]
            self.graphs = (g_fwd, g_bwd, self.graphs[2])
        self._replay(time_exposed=self._time_exposed if time_exposed else None)
        return self.loss

    def exposed_ms(self):
        """Mean time the compute stream waited for the gradient exchange after the last backward graph (call after a
        device synchronize)."""
        if not self._exposed:
            return None
        t = [a.elapsed_time(b) for a, b in self._exposed]
        self._exposed = []
        return sum(t) / len(t)
