"""The validation step of the reference's supervised loops, graph-replayed, for the live and the EMA weights.

The reference's ``validation_step`` (imagenet_classification/supervised_imagenet.py:151-210, mae/finetune_imagenet.py:165-221,
cell_imaging/supervised.py:132-165) runs every batch through the live backbone and through ``self.ema.module`` and logs
``val_loss``, ``val_acc``, ``val_loss_ema`` and ``val_acc_ema`` as epoch means summed over ranks; the accuracies its READMEs
quote are ``val_acc_ema``.  Here:

* ``EvalMetrics`` keeps loss sum, sample / correct counts and per-class counts in ONE block of device memory that
  ``fv_eval_accumulate`` (csrc/eval.hip) adds a batch to -- no host sync until ``compute()``, one small all-reduce over ranks;
* ``FlatAdamW.swap_ema_()`` / ``ema_weights(opt)`` put the EMA weights where the model's forward reads its weights (fp32
  masters, bf16 shadow and every derived copy) with one streaming launch, and take them out again bit for bit;
* ``ValidationStep`` captures  forward -> accumulate -> swap -> forward -> accumulate -> swap back  as one HIP graph next to
  the training step's graphs, with the number of valid rows of the (static) batch in device memory so that the short last
  batch of an epoch replays the same graph.
"""
import contextlib

import torch
import torch.distributed as dist

from . import _lib as L
from ._devblock import BlockWriter
from .graph_chain import capture, capture_allowed, capture_mode, warm_up

ACC_HEAD = 3             # include/fastvim_hip.h, FV_EVAL_ACC_HEAD: [loss_sum (fp64) | n_seen | n_correct] before the class counters
MAX_CLASSES = 2048       # the row kernel keeps a row in one wave's registers (csrc/ce_row.h: 64 lanes x 32)


def block_words(num_classes):
    """64-bit words of an accumulator block: ``[loss_sum | n_seen | n_correct | support[C] | hit[C]]``."""
    return ACC_HEAD + 2 * int(num_classes)


def metrics_from_counts(block, num_classes):
    """The epoch metrics of one accumulator block -- a pure host function: ``block`` is a CPU int64 tensor of
    ``block_words(num_classes)`` words (word 0 holds the bits of the fp64 loss sum).

    Returns ``{"loss", "acc_micro", "acc_macro", "n", "support", "hit"}``:

    * ``loss = loss_sum / n`` and ``acc_micro = n_correct / n``: over an epoch exactly what Lightning logs for
      ``self.log(..., on_epoch=True)`` of per-batch means -- the batch-size-weighted mean of the batch means -- and what
      torchmetrics' ``average="micro"`` accumulates (every recipe of the reference uses micro);
    * ``acc_macro``: the mean over the classes with ``support > 0`` of ``hit / support``, taken over the EPOCH's counts.  The
      reference's macro variant is a different number: torchmetrics' macro accuracy of each batch (over the classes that
      batch happens to contain), averaged over batches by Lightning.  The epoch-level definition is the meaningful one --
      it does not depend on how the set was cut into batches -- and is the one computed here;
    * ``n``: samples seen (int); ``support`` / ``hit``: (C,) int64 CPU tensors, per-class label and correct counts.  A sample
      whose label is outside ``[0, C)`` is in ``n`` and in no class.

    With ``n == 0`` (nothing accumulated since ``reset()``) ``loss`` and ``acc_micro`` are NaN -- the mean of no samples,
    as ``torch.empty(0).mean()`` -- and so is ``acc_macro`` whenever no class has support; nothing raises."""
    C = int(num_classes)
    if block.device.type != "cpu" or block.dtype != torch.int64 or block.numel() != block_words(C):
        raise ValueError(f"metrics_from_counts: a CPU int64 block of {block_words(C)} words is expected, got "
                         f"{block.dtype} x {block.numel()} on {block.device}")
    block = block.contiguous()
    loss_sum = float(block[:1].view(torch.float64).item())
    n, n_correct = int(block[1]), int(block[2])
    support = block[ACC_HEAD:ACC_HEAD + C].clone()
    hit = block[ACC_HEAD + C:ACC_HEAD + 2 * C].clone()
    nan = float("nan")
    present = support > 0
    macro = float((hit[present].double() / support[present].double()).mean()) if bool(present.any()) else nan
    return {"loss": loss_sum / n if n else nan, "acc_micro": n_correct / n if n else nan, "acc_macro": macro, "n": n,
            "support": support, "hit": hit}


def _world(group):
    return dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1


def allreduce_blocks(blocks, process_group=None):
    """Sum accumulator blocks (int64 tensors, all on one device) over the ranks of ``process_group`` in ONE all-reduce:
    the blocks travel as one fp64 vector -- the loss sums as they are, the counters converted (exact below 2**53) -- and
    come back as new int64 blocks.  One rank (or no process group): clones."""
    if _world(process_group) == 1:
        return [b.clone() for b in blocks]
    parts = []
    for b in blocks:
        b = b.contiguous()
        parts += [b[:1].view(torch.float64), b[1:].to(torch.float64)]
    wire = torch.cat(parts)
    dist.all_reduce(wire, op=dist.ReduceOp.SUM, group=process_group)
    out, o = [], 0
    for b in blocks:
        k = b.numel()
        nb = torch.empty_like(b, memory_format=torch.contiguous_format)
        nb[:1].view(torch.float64).copy_(wire[o:o + 1])
        nb[1:].copy_(wire[o + 1:o + k].round().to(torch.int64))
        out.append(nb)
        o += k
    return out


class EvalMetrics:
    """Loss and top-1 accuracy of a validation epoch, accumulated on the device.  ``update`` adds a batch with two small
    launches and no host sync; ``compute`` reads the block back once.  Cross-entropy without smoothing, the
    ``F.cross_entropy`` of the reference's ``validation_step``; at most 2048 classes."""

    def __init__(self, num_classes, device):
        self.num_classes = int(num_classes)
        if not 1 <= self.num_classes <= MAX_CLASSES:
            raise ValueError(f"EvalMetrics: 1 to {MAX_CLASSES} classes, got {num_classes}")
        self.device = torch.device(device)
        self.block = torch.zeros(block_words(self.num_classes), device=self.device, dtype=torch.int64)
        self._scratch = {}           # batch -> (loss_rows, correct_rows)
        self._nv = None              # update()'s own row count in device memory, its writer and the value it holds
        self._nv_writer = None
        self._nv_value = None

    def reset(self):
        self.block.zero_()

    def scratch(self, batch):
        s = self._scratch.get(batch)
        if s is None:
            s = self._scratch[batch] = (torch.zeros(batch, device=self.device, dtype=torch.float32),
                                        torch.zeros(batch, device=self.device, dtype=torch.int32))
        return s

    def accumulate(self, logits, labels, n_valid):
        """The two launches: ``n_valid`` is a 1-element int32 DEVICE tensor read when they run (capturable; the scratch
        of this batch size must exist before a capture -- ``scratch(batch)``)."""
        L.require_gpu(logits, labels, n_valid)
        if logits.dim() != 2 or logits.shape[1] != self.num_classes or labels.shape != logits.shape[:1]:
            raise RuntimeError(f"EvalMetrics: logits {tuple(logits.shape)} must be (B, {self.num_classes}) and labels "
                               f"{tuple(labels.shape)} (B,)")
        if labels.dtype != torch.int64:
            raise RuntimeError(f"EvalMetrics: labels must be int64 class indices, got {labels.dtype}")
        if n_valid.dtype != torch.int32 or n_valid.numel() != 1:
            raise RuntimeError("EvalMetrics: n_valid must be one int32 in device memory")
        x = logits.detach().contiguous()
        if x.dtype not in (torch.float32, torch.bfloat16):
            x = x.float()
        lab = labels.contiguous()
        B = x.shape[0]
        rows, correct = self.scratch(B)
        rc = L.lib().fv_eval_accumulate(L.ptr(x), L.i32(L.dtype_code(x.dtype)), L.ptr(lab), L.ptr(n_valid), L.ptr(rows),
                                        L.ptr(correct), L.ptr(self.block), L.i32(B), L.i32(self.num_classes), L.stream_of(x))
        L.check(rc, "eval_accumulate")

    def update(self, logits, labels, n_valid=None):
        """Eager: add the first ``n_valid`` rows (default: all) of a batch.  The count goes to the device through a pinned
        staging ring (fastvim_amd/_devblock.py), so the call does not wait for the GPU."""
        B = logits.shape[0]
        n = B if n_valid is None else int(n_valid)
        if not 0 <= n <= B:
            raise ValueError(f"EvalMetrics.update: n_valid = {n} outside [0, {B}]")
        L.require_gpu(logits, labels)
        if self._nv is None:
            self._nv = torch.zeros(1, device=self.device, dtype=torch.int32)
            self._nv_writer = BlockWriter(1)
        if n != self._nv_value:
            self._nv_writer.write(self._nv, [n])
            self._nv_value = n
        self.accumulate(logits, labels, self._nv)

    def compute(self, process_group=None):
        """One device-to-host read (it synchronises); with more than one rank the block is summed over them first, in one
        all-reduce.  Returns ``metrics_from_counts``' dictionary."""
        (blk,) = allreduce_blocks([self.block], process_group)
        return metrics_from_counts(blk.cpu(), self.num_classes)


@contextlib.contextmanager
def ema_weights(opt):
    """``with ema_weights(opt): logits = model(x)`` -- the model computes with the optimizer's EMA weights inside the block
    and with its own again after it: two ``FlatAdamW.swap_ema_()`` launches, which restore ``param_flat``, ``ema``,
    ``shadow_flat`` and every derived copy bit for bit."""
    opt.swap_ema_()
    try:
        yield opt
    finally:
        opt.swap_ema_()


@contextlib.contextmanager
def _eval_mode(model):
    """``model.eval()`` inside, every module's own ``training`` flag put back after."""
    flags = [(m, m.training) for m in model.modules()]
    model.eval()
    try:
        yield
    finally:
        for m, t in flags:
            m.training = t


class ValidationStep:
    """The reference's ``validation_step`` as one HIP graph.  ``model`` / ``flat`` / ``opt`` are the training step's;
    ``x`` and ``labels`` ((B,) int64) are the static input buffers: copy a batch into their first ``n`` rows and call
    ``step(n_valid=n)``.

        forward (live weights) -> accumulate -> swap -> forward (EMA weights) -> accumulate -> swap back

    The forward is the evaluation forward (DropPath off, every channel of the channel models) under ``torch.no_grad()``
    and ``amp_dtype`` autocast; a single chain of launches on one stream, captured into a memory pool of its own.
    ``ema=False`` runs the live half only (also what an optimizer without EMA weights, ``FlatSGD``, gets); ``ema=True``
    with such an optimizer raises.  Neither construction nor ``step()`` changes ``model.training``, the CPU / GPU RNG
    streams, or any buffer of the flat state and the optimizer (the two swaps of a step cancel bit for bit), so steps can
    be interleaved with training steps anywhere between two of them.

    ``compute()`` returns ``val_loss``, ``val_acc``, ``val_acc_macro``, ``n`` and, with ``ema``, ``val_loss_ema``,
    ``val_acc_ema``, ``val_acc_macro_ema`` (``metrics_from_counts`` defines them); ``reset()`` starts the next epoch."""

    def __init__(self, model, flat, opt, x, labels, amp_dtype=torch.bfloat16, use_graph=True, ema=True, warmup=1):
        if ema and getattr(opt, "ema", None) is None:
            raise RuntimeError("ValidationStep(ema=True): the optimizer holds no EMA weights -- build FlatAdamW with "
                               "ema_decay=..., or pass ema=False to validate the live weights only")
        L.require_gpu(x, labels)
        if labels.dtype != torch.int64 or labels.shape != x.shape[:1]:
            raise RuntimeError(f"ValidationStep: labels must be ({x.shape[0]},) int64, got {tuple(labels.shape)} {labels.dtype}")
        self.model, self.flat, self.opt = model, flat, opt
        self.x, self.labels, self.amp_dtype, self.ema = x, labels, amp_dtype, bool(ema)
        self.batch = x.shape[0]
        self._nv = torch.full((1,), self.batch, device=x.device, dtype=torch.int32)
        self._nv_writer = BlockWriter(1)
        self._nv_value = self.batch
        self.live = self.ema_metrics = None
        self.use_graph = use_graph
        self.graph = None
        dev = x.device
        cpu_rng, gpu_rng = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
        with _eval_mode(model):
            # the first forward tells the number of classes; it and the warm-up steps run on a side stream, as a capture
            # wants (with use_graph=False too), and what they add to the metrics is zeroed again
            classes = warm_up(self._forward, 1, dev).shape[1]
            self.live = EvalMetrics(classes, dev)
            self.live.scratch(self.batch)
            if self.ema:
                self.ema_metrics = EvalMetrics(classes, dev)
                self.ema_metrics.scratch(self.batch)
            warm_up(self._sequence, max(int(warmup), 1) if use_graph else int(warmup), dev)
            self.reset()
            torch.cuda.synchronize(dev)
            if use_graph:
                self._capture()
        torch.set_rng_state(cpu_rng)
        torch.cuda.set_rng_state(gpu_rng, dev)

    # ------------------------------------------------------------------ the pieces
    def _forward(self):
        with torch.no_grad(), torch.autocast("cuda", dtype=self.amp_dtype, enabled=self.amp_dtype != torch.float32):
            return self.model(self.x)

    def _sequence(self):
        self.live.accumulate(self._forward(), self.labels, self._nv)
        if self.ema:
            with ema_weights(self.opt):
                self.ema_metrics.accumulate(self._forward(), self.labels, self._nv)

    def _capture(self):
        if not capture_allowed("ValidationStep"):
            self.use_graph = False
            return
        self.graph, _ = capture(torch.cuda.graph_pool_handle(), capture_mode(), self._sequence)

    # ------------------------------------------------------------------ run
    def step(self, n_valid=None):
        """Evaluate the first ``n_valid`` rows (default: all) of the static batch under both weight sets and add them to
        the metrics.  Returns nothing: nothing here waits for the GPU."""
        n = self.batch if n_valid is None else int(n_valid)
        if not 0 <= n <= self.batch:
            raise ValueError(f"ValidationStep.step: n_valid = {n} outside [0, {self.batch}]")
        if n != self._nv_value:
            self._nv_writer.write(self._nv, [n])
            self._nv_value = n
        if self.graph is not None:
            self.graph.replay()
        else:
            with _eval_mode(self.model):
                self._sequence()

    def reset(self):
        self.live.reset()
        if self.ema_metrics is not None:
            self.ema_metrics.reset()

    def compute(self, process_group=None):
        """One device-to-host read; with more than one rank, one all-reduce of both blocks first."""
        blocks = [self.live.block] + ([self.ema_metrics.block] if self.ema else [])
        blocks = torch.stack(allreduce_blocks(blocks, process_group)).cpu()
        C = self.live.num_classes
        m = metrics_from_counts(blocks[0], C)
        out = {"val_loss": m["loss"], "val_acc": m["acc_micro"], "val_acc_macro": m["acc_macro"], "n": m["n"]}
        if self.ema:
            e = metrics_from_counts(blocks[1], C)
            out.update({"val_loss_ema": e["loss"], "val_acc_ema": e["acc_micro"], "val_acc_macro_ema": e["acc_macro"]})
        return out
