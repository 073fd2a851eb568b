"""What the graph-replayed steps share: the capture helpers every step uses (``pipeline.SegmentedTrainStep``,
``mae_step.MAEPretrainStep``, ``linear_probe.LinearProbeStep``, ``evaluate.ValidationStep``) and ``ChainStep``, the chain
of forward / per-run backward / optimizer graphs with the gradient exchange between them that the first two are.  The
order of captures and replays lives here, once ("The graph-chain scaffold")."""
import functools
import warnings

import torch
import torch.distributed as dist


# ---------------------------------------------------------------------------------------------------- capture helpers
def capture_mode():
    """The ``capture_error_mode`` every capture here uses."""
    # With a process group alive, its watchdog THREAD polls the events of finished collectives (hipEventQuery); under the
    # default "global" capture mode any thread's event query while this thread captures is an error
    # (hipErrorStreamCaptureUnsupported: "operation not permitted when stream is capturing" -- it took the whole process
    # down, intermittently, in tests/test_pipeline_gpu.py::test_rccl_buckets_between_backward_graphs).  "thread_local"
    # restricts the check to the capturing thread, which issues nothing but kernel launches.
    return "thread_local" if (dist.is_available() and dist.is_initialized()) else "global"


def capture_allowed(who):
    """False (after one ``RuntimeWarning`` in the name of the class ``who``) when the step must run eagerly.  Call it from
    the method the step's constructor calls: the warning then points at the line that builds the step."""
    from . import graph_capture_safe
    if graph_capture_safe():
        return True
    # known to replay some captured steps wrongly (non-finite after a few replays): do not capture at all
    warnings.warn(f"{who}: HIP was initialised before `import fastvim_amd` could switch graph packet capture off "
                  "(DEBUG_CLR_GRAPH_PACKET_CAPTURE=0): on ROCm 7.2 some captured training steps replay wrongly (DESIGN.md "
                  "section 5) -- running this step EAGERLY instead.  Import fastvim_amd first, or export the variable, to "
                  "get graph replay.", RuntimeWarning, stacklevel=4)
    return False


def warm_up(fn, n, device=None):
    """``fn()`` n times on a side stream, as a capture wants its warm-up (allocator, lazily built buffers, RCCL
    communicators); the stream is joined back and the device synchronised.  Returns what the last call returned."""
    out = None
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        for _ in range(n):
            out = fn()
    torch.cuda.current_stream(device).wait_stream(side)
    torch.cuda.synchronize(device)
    return out


def capture(pool, mode, *pieces):
    """One graph of ``pieces`` called in order -> (graph, the last result that is not None)."""
    g, out = torch.cuda.CUDAGraph(), None
    with torch.cuda.graph(g, pool=pool, capture_error_mode=mode):
        for piece in pieces:
            r = piece()
            out = r if r is not None else out
    return g, out


def snapshot_training_state(flat, opt, extra=()):
    """What the warm-up steps of a capture may advance, cloned: (buffers, CPU RNG state, GPU RNG state, device) for
    ``restore_training_state``.  ``extra``: further buffers of the caller's (the probe's BatchNorm statistics)."""
    f, o = flat, opt
    # every tensor attribute of the optimizer (moments, EMA, step count, lr, decay mask, ...) and the state's own buffers:
    # whatever a warm-up step may advance is put back, not a hand-picked list
    bufs = [f.param_flat, f.shadow_flat] + list(getattr(f, "_t_dst", [])) + list(getattr(f, "_tx_dst", [])) + list(getattr(f, "_pk_dst", []))   # (+ the transposed in_proj / x_proj shadows and the fragment-major copies)
    bufs += list(extra)
    for v in vars(o).values():
        if torch.is_tensor(v) and v.is_cuda and all(v is not b for b in bufs):
            bufs.append(v)
    dev = f.param_flat.device
    return [(b, b.clone()) for b in bufs], torch.get_rng_state(), torch.cuda.get_rng_state(dev), dev


def restore_training_state(snap):
    bufs, cpu_rng, gpu_rng, dev = snap
    with torch.no_grad():
        for b, saved in bufs:
            b.copy_(saved)
    torch.set_rng_state(cpu_rng)
    torch.cuda.set_rng_state(gpu_rng, dev)


# ---------------------------------------------------------------------------------------------------- the chain
def run_chain(fwd, bwd, opt, ex, exchange=True, time_exposed=None):
    """The order of one pass, eager (``fwd`` / ``bwd[k]`` / ``opt`` are the step's own functions) or replayed (the graphs'
    ``replay``):  fwd -> (bwd k, launch(bucket k))* -> finish() -> opt.  ``exchange=False`` (a micro-batch that is not the
    last of its group) stops after the backward runs: nothing is launched, finished or stepped.  ``time_exposed``: a
    context manager factory put around ``finish``.  Only host calls of the arguments: ``ex.launch`` / ``ex.finish`` are
    looked up when they are called.  Returns what ``fwd`` returned."""
    loss = fwd()
    for k, b in enumerate(bwd):
        b()
        if exchange:
            ex.launch(k)
    if exchange:
        if time_exposed is None:
            ex.finish(mean=False)        # sums: the optimizer kernel applies its gradient scale as it reads them
        else:
            with time_exposed():
                ex.finish(mean=False)
        opt()
    return loss


class ChainStep:
    """The block stack cut into K runs: ONE forward graph, K backward graphs of one run each (last run first), one optimizer
    graph, bucket k's exchange launched behind backward graph k.  A subclass supplies ``_forward()`` -- built on
    ``_run_cuts`` / ``_end_forward`` -- and may extend ``_snapshot`` / ``_restore`` / ``_warm_step`` / ``_capture_families``;
    it calls ``_capture(warmup)`` from its constructor when ``use_graph`` is set."""

    def __init__(self, flat, opt, x, n_segments, use_graph, accum_iter=1):
        self.flat, self.opt, self.x = flat, opt, x
        self.exchange = flat.make_exchange(n_segments)
        self.runs = self.exchange.layers                 # (lo, hi) block ranges in BACKWARD order
        self.K = len(self.runs)
        self._gscale = 1.0 / (accum_iter * self.exchange.world_size)
        self.use_graph = use_graph
        self.loss = None
        self._seed = torch.ones((), device=x.device, dtype=torch.float32)      # d loss / d loss, allocated once outside the graphs
        self._cuts = None
        self.graphs = None

    # ------------------------------------------------------------------ the pieces
    def _run_cuts(self, run, carry):
        """The runs in forward order: ``carry = run(lo, hi, *carry)``.  The first two entries of ``carry`` are the
        activations that cross a cut -- each run's inputs are leaves that alias the previous run's outputs -- and whatever
        follows them is handed on as it is.  Returns the last run's ``carry``."""
        cuts = []              # per run in FORWARD order: (inputs (leaves) or None, outputs)
        for i, (lo, hi) in enumerate(self.runs[::-1]):
            ins = None
            if i > 0:
                ins = tuple(t.detach().requires_grad_() for t in carry[:2])
                carry = ins + tuple(carry[2:])
            carry = run(lo, hi, *carry)
            cuts.append([ins, tuple(carry[:2])])
        self._cuts = cuts
        return carry

    def _end_forward(self, loss):
        self._cuts[-1][1] = (loss,)
        return loss.detach()

    def _backward(self, k):
        """Backward of run k (backward order: k = 0 is the last run of blocks, whatever follows it and the loss)."""
        i = self.K - 1 - k                      # forward index
        outs = self._cuts[i][1]
        if k == 0:
            seed = self._seed if (outs[0].dim() == 0 and outs[0].dtype == self._seed.dtype and outs[0].device == self._seed.device) else None
            torch.autograd.backward(outs[0], seed)      # (the seed autograd would otherwise fill inside the captured graph)
        else:
            nxt = self._cuts[i + 1][0]
            torch.autograd.backward(list(outs), [t.grad for t in nxt])
        self.flat.finish_backward()             # this run's queued weight-gradient GEMMs and partial sums
        self._cuts[i][1] = None                 # free the run's autograd graph

    def _optimize(self):
        self.opt.step(grad_scale=self._gscale)

    # ------------------------------------------------------------------ capture
    def _snapshot(self):
        return snapshot_training_state(self.flat, self.opt)

    def _restore(self, snap):
        restore_training_state(snap[:4])

    def _warm_step(self):
        self._eager()

    def _capture_family(self, warmup, snap, pool, mode):
        """Warm up with whole eager steps, put back what they advanced, capture -> (forward graph, backward graphs, loss)."""
        warm_up(self._warm_step, warmup)
        self._restore(snap)
        torch.cuda.synchronize()
        g_fwd, loss = capture(pool, mode, self._forward)
        g_bwd = [capture(pool, mode, functools.partial(self._backward, k))[0] for k in range(self.K)]
        return g_fwd, g_bwd, loss

    def _capture_families(self, warmup, snap, pool, mode):
        return self._capture_family(warmup, snap, pool, mode)       # (a step with more than one family overrides this)

    def _capture(self, warmup):
        if not capture_allowed(type(self).__name__):
            self.use_graph = False
            return
        snap, pool, mode = self._snapshot(), torch.cuda.graph_pool_handle(), capture_mode()
        g_fwd, g_bwd, self.loss = self._capture_families(warmup, snap, pool, mode)
        self.graphs = (g_fwd, g_bwd, capture(pool, mode, self._optimize)[0])

    # ------------------------------------------------------------------ run
    def _eager(self, exchange=True):
        return run_chain(self._forward, [functools.partial(self._backward, k) for k in range(self.K)], self._optimize,
                         self.exchange, exchange)

    def _replay(self, exchange=True, time_exposed=None):
        g_fwd, g_bwd, g_opt = self.graphs
        run_chain(g_fwd.replay, [g.replay for g in g_bwd], g_opt.replay, self.exchange, exchange, time_exposed)
