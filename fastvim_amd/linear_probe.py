"""Linear probing of a frozen backbone on the HIP path (reference recipe: mae/linear.py, mae/linear_imagenet.py,
mae/lars.py, mae/config/linear_FastVimL.yaml).

The recipe replaces ``backbone.head`` by ``Sequential(BatchNorm1d(d, affine=False, eps=1e-6), head)``, freezes everything
but the head and trains it with momentum SGD (LARS in the recipe it was derived from).  Here:

* ``ProbeBatchNorm1d`` -- ``nn.BatchNorm1d`` (same constructor, buffers, ``state_dict`` keys) on three kernels
  (csrc/bn1d.hip): per-column statistics of this rank's rows, [all-gather of one table row per rank,] normalise + running
  statistics, and the adjoint;
* ``attach_probe_head`` -- what ``SupervisedModule.__init__`` (linear_imagenet.py:39-53) does to the model;
* ``freeze_shadows`` -- compute-dtype copies of the frozen projection weights, so a frozen forward casts nothing;
* ``LinearProbeStep`` -- the graph-replayed step: backbone under ``no_grad``, BatchNorm, head GEMM, cross-entropy, backward
  over the head only, ``FlatSGD`` (fastvim_amd/flat.py).

The recipe's learning-rate schedule (linear_imagenet.py:118-130), set between steps with ``opt.set_lr``::

    epoch = current_epoch + batch_idx / batches_per_epoch
    lr = base_lr * epoch / warmup_epochs if epoch < warmup_epochs else \\
        min_lr + (base_lr - min_lr) * 0.5 * (1 + math.cos(math.pi * (epoch - warmup_epochs) / (epochs - warmup_epochs)))
    opt.set_lr(lr); x.copy_(images); labels.copy_(targets); loss = step.step()
"""
import torch
import torch.distributed as dist
import torch.nn as nn

from . import _lib as L
from .gemm import gemm_any_nn, gemm_any_nt
from .glue_ops import column_sum
from .graph_chain import capture, capture_allowed, capture_mode, restore_training_state, snapshot_training_state, warm_up
from .losses import CrossEntropyLoss
from .mamba_simple_faster import _compute_dtype, _direct_grad, _shadow, _wgrad


# ---------------------------------------------------------------------------------------------------- kernel wrappers
def _feature_tensor(x, what):
    L.require_gpu(x)
    if x.dim() != 2:
        raise ValueError(f"{what}: expected (batch, features) input, got {tuple(x.shape)}")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"{what}: features must be fp32 or bf16, got {x.dtype}")
    return x.contiguous()


def bn1d_stats(x, out=None):
    """One table row ``[mean(d) | M2(d) | count]`` (fp32, 2 d + 1) of the rows of ``x`` (B, d): ``fv_bn1d_stats``."""
    x = _feature_tensor(x.detach(), "bn1d_stats")
    B, d = x.shape
    if out is None:
        out = torch.empty(2 * d + 1, device=x.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.numel() == 2 * d + 1 and out.is_contiguous()
    rc = L.lib().fv_bn1d_stats(L.ptr(x), L.i32(L.dtype_code(x.dtype)), L.ptr(out), L.i32(B), L.i32(d), L.stream_of(x))
    L.check(rc, "bn1d_stats")
    return out


def bn1d_apply(x, table, running_mean, running_var, num_batches_tracked, eps, momentum, training):
    """``fv_bn1d_apply``: ``table`` (world, 2 d + 1) rows in rank order (training), or None (eval: running statistics).
    Returns ``(xhat, mean, rstd)``; in training mode the running buffers and the counter are advanced on the device."""
    import ctypes
    x = _feature_tensor(x.detach(), "bn1d_apply")
    B, d = x.shape
    world = 0
    if training:
        table = table.view(-1, 2 * d + 1)
        assert table.dtype == torch.float32 and table.is_contiguous() and table.device == x.device
        world = table.shape[0]
    for b in (running_mean, running_var):
        assert b is None or (b.dtype == torch.float32 and b.numel() == d and b.is_contiguous() and b.device == x.device)
    assert num_batches_tracked is None or (num_batches_tracked.dtype == torch.int64 and num_batches_tracked.device == x.device)
    xhat = torch.empty_like(x)
    mean = torch.empty(d, device=x.device, dtype=torch.float32)
    rstd = torch.empty(d, device=x.device, dtype=torch.float32)
    rc = L.lib().fv_bn1d_apply(L.ptr(x), L.i32(L.dtype_code(x.dtype)), L.ptr(table if training else None), L.i32(world),
                               L.ptr(running_mean), L.ptr(running_var), L.ptr(num_batches_tracked), L.ptr(xhat), L.ptr(mean),
                               L.ptr(rstd), L.i32(B), L.i32(d), ctypes.c_float(eps), ctypes.c_float(momentum),
                               L.i32(1 if training else 0), L.stream_of(x))
    L.check(rc, "bn1d_apply")
    return xhat, mean, rstd


def bn1d_bwd(dy, x, mean, rstd, training):
    """``fv_bn1d_bwd``: the input gradient of a single process's BatchNorm1d (``training``: batch statistics)."""
    x = _feature_tensor(x.detach(), "bn1d_bwd")
    dy = dy.to(x.dtype).contiguous()
    B, d = x.shape
    dx = torch.empty_like(x)
    rc = L.lib().fv_bn1d_bwd(L.ptr(dy), L.ptr(x), L.i32(L.dtype_code(x.dtype)), L.ptr(mean), L.ptr(rstd), L.ptr(dx), L.i32(B),
                             L.i32(d), L.i32(1 if training else 0), L.stream_of(x))
    L.check(rc, "bn1d_bwd")
    return dx


def gather_table(row, table, group=None):
    """All-gather one statistics row per rank into ``table`` (world, 2 d + 1), rows in rank order -- the only exchange a
    synchronised BatchNorm forward needs (mean, M2 and count travel together).  Works on CPU tensors (gloo) and GPU
    tensors (RCCL); returns ``table``."""
    world = dist.get_world_size(group)
    table = table.view(world, row.numel())
    if row.is_cuda:
        dist.all_gather_into_tensor(table.view(-1), row, group=group)
    else:
        dist.all_gather(list(table.unbind(0)), row, group=group)
    return table


def _world(group):
    return dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1


class _BatchNorm1dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, table, running_mean, running_var, num_batches_tracked, eps, momentum, training):
        xc = _feature_tensor(x.detach(), "ProbeBatchNorm1d")
        xhat, mean, rstd = bn1d_apply(xc, table, running_mean, running_var, num_batches_tracked, eps, momentum, training)
        ctx.training = training
        if x.requires_grad:
            ctx.save_for_backward(xc, mean, rstd)
        return xhat

    @staticmethod
    def backward(ctx, dy):
        xc, mean, rstd = ctx.saved_tensors
        return bn1d_bwd(dy, xc, mean, rstd, ctx.training), None, None, None, None, None, None, None


class ProbeBatchNorm1d(nn.BatchNorm1d):
    """``nn.BatchNorm1d`` over (batch, features) inputs on the HIP kernels.  ``process_group``: the ranks the batch
    statistics are taken over (None: the default group when ``torch.distributed`` is initialised -- the recipe trains with
    ``sync_batchnorm=True``, mae/linear.py:41); with more than one rank the per-rank table rows are all-gathered between
    the statistics launch and the normalising launch.  Not built: ``affine=True``, ``momentum=None`` (cumulative average),
    (N, C, L) inputs and the input gradient across ranks -- each raises."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, device=None, dtype=None,
                 process_group=None):
        super().__init__(num_features, eps=eps, momentum=momentum, affine=affine, track_running_stats=track_running_stats,
                         device=device, dtype=dtype)
        self.process_group = process_group

    def _check(self, x):
        L.require_gpu(x)
        if x.dim() != 2:
            raise ValueError(f"ProbeBatchNorm1d: expected (batch, features) input, got {tuple(x.shape)}")
        if x.shape[1] != self.num_features:
            raise ValueError(f"ProbeBatchNorm1d: expected {self.num_features} features, got {x.shape[1]}")
        if self.affine:
            raise NotImplementedError("ProbeBatchNorm1d: affine=True is not built (the probe head uses affine=False)")
        if self.momentum is None:
            raise NotImplementedError("ProbeBatchNorm1d: momentum=None (cumulative moving average) is not built")

    def uses_batch_stats(self):
        return self.training or self.running_mean is None

    def local_stats(self, x, out=None):
        """This rank's table row of ``x`` (the first of the two launches)."""
        self._check(x)
        return bn1d_stats(x if x.dtype in (torch.float32, torch.bfloat16) else x.float(), out)

    def normalize(self, x, table=None):
        """The second launch: ``table`` holds one row per rank (batch statistics), or is None (running statistics)."""
        self._check(x)
        if x.dtype not in (torch.float32, torch.bfloat16):
            x = x.float()
        batch = self.uses_batch_stats()
        if batch and table is None:
            raise ValueError("ProbeBatchNorm1d.normalize: batch statistics need the table of local_stats rows")
        if batch and table.numel() > 2 * self.num_features + 1 and x.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("ProbeBatchNorm1d: the input gradient across ranks (SyncBatchNorm backward) is not built")
        upd = self.training and self.track_running_stats
        return _BatchNorm1dFn.apply(x, table if batch else None, self.running_mean if (upd or not batch) else None,
                                    self.running_var if (upd or not batch) else None,
                                    self.num_batches_tracked if upd else None, float(self.eps), float(self.momentum), batch)

    def forward(self, x):
        self._check(x)
        if not self.uses_batch_stats():
            return self.normalize(x)
        world = _world(self.process_group)
        if world == 1 and x.shape[0] == 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
        row = self.local_stats(x)
        if world > 1:
            row = gather_table(row, torch.empty(world, row.numel(), device=row.device, dtype=row.dtype), self.process_group)
        return self.normalize(x, row)


# ---------------------------------------------------------------------------------------------------- the probe head
def is_probe_head(head):
    return isinstance(head, nn.Sequential) and len(head) == 2 and isinstance(head[0], ProbeBatchNorm1d) \
        and isinstance(head[1], nn.Linear)


class ProbeLinearFn(torch.autograd.Function):
    """The probe's linear layer, ``logits = xhat @ W^T + b``, with fp32 logits and an fp32 logit gradient whatever the
    compute dtype: operands in the compute dtype (xhat as the BatchNorm wrote it, W from its shadow), products and sums in
    fp32 on the fp32-MFMA GEMM (csrc/gemm_f32.hip) -- in fp32 exactly what ``LinearFn`` launches; under bf16 autocast
    ``LinearFn`` would round the logits and their gradient to bf16, which for ten-to-a-thousand logits per row buys
    nothing and costs the head's gradient 8 bits.  dW (deterministic split-K) and db go straight into the flat
    gradient, like ``LinearFn``'s."""

    @staticmethod
    def forward(ctx, a, W, cdt, bias=None):
        with torch.autocast("cuda", enabled=False):
            a2 = a.reshape(-1, a.shape[-1]).to(cdt).contiguous()
            y = gemm_any_nt(a2, _shadow(W, cdt), bias, out_dtype=torch.float32)
        ctx.save_for_backward(a2, W)
        ctx.a_shape, ctx.a_dtype, ctx.cdt = a.shape, a.dtype, cdt
        ctx.need_da = a.requires_grad
        ctx.bias_ref = bias
        return y.view(*a.shape[:-1], W.shape[0])

    @staticmethod
    def backward(ctx, g):
        a2, W = ctx.saved_tensors
        with torch.autocast("cuda", enabled=False):
            g2 = g.reshape(-1, g.shape[-1]).float().contiguous()
            da = None
            if ctx.need_da:
                da = gemm_any_nn(g2, _shadow(W, ctx.cdt), out_dtype=ctx.a_dtype).view(ctx.a_shape)
            dW = _wgrad(g2, a2, W)
            if dW is not None:
                dW = dW.view(W.shape)
            db = None
            bias = ctx.bias_ref
            if bias is not None:
                gd = _direct_grad(bias)
                if gd is not None:
                    column_sum(g2, out=gd.view(-1), accumulate=True)
                else:
                    db = column_sum(g2)
        return da, dW, None, db


def probe_linear(linear, xhat):
    return ProbeLinearFn.apply(xhat, linear.weight, _compute_dtype(xhat), linear.bias)


def probe_head_forward(head, x):
    """``head(x)`` for the probe head: the BatchNorm kernels, then the project's own GEMM (fp32 logits)."""
    return probe_linear(head[1], head[0](x))


def attach_probe_head(model, process_group=None):
    """What ``SupervisedModule.__init__`` does to its backbone (mae/linear_imagenet.py:39-53): re-draw the head weight
    (``trunc_normal_(std=0.01)``), put a ``BatchNorm1d(in_features, affine=False, eps=1e-6)`` in front of it, freeze every
    parameter and un-freeze the head's.  A reference linear-probe checkpoint then loads by key (``head.0.running_mean``,
    ``head.0.running_var``, ``head.0.num_batches_tracked``, ``head.1.weight``, ``head.1.bias``).  Call it BEFORE a
    ``FlatTrainingState`` is attached: the flat state lays out the parameters that are trainable when it is built."""
    head = model.head
    if not isinstance(head, nn.Linear):
        raise TypeError(f"attach_probe_head: model.head must be an nn.Linear, got {type(head).__name__}")
    with torch.no_grad():
        nn.init.trunc_normal_(head.weight, std=0.01, a=-2.0, b=2.0)      # timm.layers.trunc_normal_(w, std=0.01)
    bn = ProbeBatchNorm1d(head.in_features, affine=False, eps=1e-6, device=head.weight.device, process_group=process_group)
    model.head = nn.Sequential(bn, head)
    for p in model.parameters():
        p.requires_grad = False
    for p in model.head.parameters():
        p.requires_grad = True
    return model


def freeze_shadows(model, dtype=torch.bfloat16):
    """One flat buffer of ``dtype`` copies of the frozen weights the forward pass asks ``_shadow()`` for -- the weights of
    the ``nn.Linear`` and ``nn.Conv2d`` modules (in_proj, out_proj, the patch projection, a frozen head) except the
    mixers' ``x_proj`` / ``dt_proj`` pairs, which the mixer stacks and reads itself -- hung on the parameters as
    ``_fv_shadow`` / ``_fv_shadow_version``: a frozen forward under ``dtype`` autocast then casts no projection weight
    (at FastVim-L: 12.6 M elements per block, every forward).  An in-place write to a parameter (``load_state_dict``)
    bumps its version counter and ``_shadow()`` re-casts that copy, as for a flat training state; trainable parameters
    are left alone (they belong to a ``FlatTrainingState``).  Returns the buffer."""
    ws = []
    for name, mod in model.named_modules():
        w = getattr(mod, "weight", None)
        leaf = name.rsplit(".", 1)[-1]
        if isinstance(mod, (nn.Linear, nn.Conv2d)) and isinstance(w, nn.Parameter) and not w.requires_grad \
                and not leaf.startswith(("x_proj", "dt_proj")) and all(w is not q for q in ws):
            ws.append(w)
    if not ws:
        return None
    offs, off = [], 0
    for w in ws:
        offs.append(off)
        off += (w.numel() + 7) // 8 * 8            # 16-byte aligned views (MFMA GEMM loads)
    buf = torch.zeros(off, device=ws[0].device, dtype=dtype)
    with torch.no_grad():
        for w, o in zip(ws, offs):
            sh = buf[o:o + w.numel()].view_as(w)
            sh.copy_(w)
            w._fv_shadow = sh
            w._fv_shadow_version = w._version
    return buf


# ---------------------------------------------------------------------------------------------------- the step
class LinearProbeStep:
    """One linear-probe training step, graph-replayed.  ``model`` carries the probe head (``attach_probe_head``) and
    ``forward_features``; ``flat`` is the ``FlatTrainingState`` over the head, ``opt`` a ``FlatSGD`` (or any fused flat
    optimizer).  ``x`` / ``labels`` ((B,) int64) are the static input buffers: copy new batches into them between steps.

        backbone (no_grad) -> statistics launch [-> all-gather of the table] -> normalise + running statistics ->
        head GEMM -> cross-entropy -> head backward (dW, db straight into the flat gradient) [-> all-reduce] -> optimizer

    One rank: one graph.  More ranks (or ``sync=True``, which runs the collectives whatever the world size): three graphs
    -- features + statistics, head + loss + backward, optimizer -- with the two collectives between them.  Construction
    runs ``warmup`` real steps and puts back everything they touched (head parameters, shadow, optimizer state, running
    statistics, ``num_batches_tracked``, RNG streams), like ``SegmentedTrainStep``."""

    def __init__(self, model, flat, opt, x, labels, amp_dtype=torch.bfloat16, use_graph=True, warmup=2, sync=None):
        if not is_probe_head(getattr(model, "head", None)):
            raise TypeError("LinearProbeStep: model.head is not a probe head -- call attach_probe_head(model) first")
        self.model, self.flat, self.opt = model, flat, opt
        self.x, self.labels, self.amp_dtype = x, labels, amp_dtype
        self.bn, self.linear = model.head[0], model.head[1]
        if not self.bn.training:
            raise RuntimeError("LinearProbeStep: the probe BatchNorm is in eval mode -- call model.train() (the reference "
                               "trains the probe with the whole module in training mode)")
        self.group = flat.group
        self.world = _world(self.group)
        self.sync = self.world > 1 if sync is None else bool(sync)
        if self.sync and not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("LinearProbeStep(sync=True) needs an initialised torch.distributed process group")
        self._gscale = 1.0 / self.world
        self.crit = CrossEntropyLoss()
        self._seed = torch.ones((), device=x.device, dtype=torch.float32)
        d = self.bn.num_features
        self._row = torch.zeros(2 * d + 1, device=x.device, dtype=torch.float32)
        self._table = torch.zeros(self.world, 2 * d + 1, device=x.device, dtype=torch.float32) if self.sync else self._row
        self._feats = None
        self.loss = None
        self.use_graph = use_graph
        self.graphs = None
        if use_graph:
            self._capture(warmup)

    # ------------------------------------------------------------------ the pieces
    def _features(self):
        with torch.no_grad(), torch.autocast("cuda", dtype=self.amp_dtype, enabled=self.amp_dtype != torch.float32):
            self._feats = self.model.forward_features(self.x)
            self.bn.local_stats(self._feats, out=self._row)

    def _gather(self):
        if self.sync:
            gather_table(self._row, self._table, self.group)

    def _head(self):
        self.flat.zero_grad()
        with torch.autocast("cuda", dtype=self.amp_dtype, enabled=self.amp_dtype != torch.float32):
            xh = self.bn.normalize(self._feats, self._table)
            logits = probe_linear(self.linear, xh)
        loss = self.crit(logits, self.labels)
        torch.autograd.backward(loss, self._seed)
        self.flat.finish_backward()
        self._feats = None
        return loss.detach()

    def _reduce(self):
        if not self.sync:
            return
        if self.world > 1:
            self.flat.allreduce_sum_()
        else:
            dist.all_reduce(self.flat.grad_flat, op=dist.ReduceOp.SUM, group=self.group)

    def _optimize(self):
        self.opt.step(grad_scale=self._gscale)

    def _eager_step(self):
        self._features()
        self._gather()
        loss = self._head()
        self._reduce()
        self._optimize()
        return loss

    # ------------------------------------------------------------------ capture / run
    def _capture(self, warmup):
        if not capture_allowed("LinearProbeStep"):
            self.use_graph = False
            return
        bn = self.bn
        snap = snapshot_training_state(self.flat, self.opt, extra=[b for b in (bn.running_mean, bn.running_var,
                                                                                bn.num_batches_tracked) if b is not None])
        pool, mode = torch.cuda.graph_pool_handle(), capture_mode()
        warm_up(self._eager_step, warmup)
        restore_training_state(snap)
        torch.cuda.synchronize()
        if not self.sync:
            g, self.loss = capture(pool, mode, self._features, self._head, self._optimize)
            self.graphs = (g,)
        else:
            g0, _ = capture(pool, mode, self._features)
            g1, self.loss = capture(pool, mode, self._head)
            g2, _ = capture(pool, mode, self._optimize)
            self.graphs = (g0, g1, g2)

    def step(self):
        """One training step; returns the (device) loss tensor."""
        if not self.use_graph:
            self.loss = self._eager_step()
            return self.loss
        if not self.sync:
            self.graphs[0].replay()
        else:
            self.graphs[0].replay()
            self._gather()
            self.graphs[1].replay()
            self._reduce()
            self.graphs[2].replay()
        return self.loss
