"""fp64 reference of the validation metrics (fastvim_amd/evaluate.py, csrc/eval.hip) and the input builders the tests
share.  Everything here is plain torch on the CPU."""
import torch


def make_batch(B, C, dtype, n_valid, seed, device="cpu"):
    """Logits whose row maximum is unique (one chosen class per row at rowmax + 1 -- the label itself in about half the
    rows -- as tests/test_mixup_gpu.py::test_top1_exact does: random bf16 rows tie otherwise and the reference itself would
    be ambiguous), labels in [0, C); the rows at and beyond ``n_valid`` hold large finite garbage and the label -1."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, C, generator=g) * 3).to(dtype)
    labels = torch.randint(0, C, (B,), generator=g)
    chosen = torch.where(torch.rand(B, generator=g) < 0.5, labels, torch.randint(0, C, (B,), generator=g))
    x[torch.arange(B), chosen] = (x.float().max(dim=1).values + 1).to(dtype)
    assert torch.equal(x.float().argmax(1), chosen)
    x[n_valid:] = torch.tensor(3.0e38).to(dtype) * torch.where(torch.rand(B - n_valid, C, generator=g) < 0.5, -1.0, 1.0).to(dtype)
    labels[n_valid:] = -1
    return x.to(device), labels.to(device)


def reference(logits, labels, n_valid, num_classes):
    """The first ``n_valid`` rows in fp64, from the STORED logits: per-row cross-entropy ``logsumexp(x) - x[label]``, the
    arg-max, and the counts.  A label outside [0, C) marks no class: the row's loss is 0 (the one-hot target is all zero),
    it is never correct and is counted in ``n`` only."""
    C = int(num_classes)
    x = logits[:n_valid].detach().cpu().double()
    y = labels[:n_valid].detach().cpu()
    ok = (y >= 0) & (y < C)
    rows = torch.zeros(n_valid, dtype=torch.float64)
    if n_valid:
        nll = torch.logsumexp(x, 1) - x.gather(1, y.clamp(0, C - 1)[:, None])[:, 0]
        rows = torch.where(ok, nll, torch.zeros_like(nll))
    correct = ok & (x.argmax(1) == y) if n_valid else torch.zeros(0, dtype=torch.bool)
    return {"loss_rows": rows, "loss_sum": float(rows.sum()), "n": int(n_valid), "n_correct": int(correct.sum()),
            "support": torch.bincount(y[ok], minlength=C), "hit": torch.bincount(y[correct], minlength=C)}


def merge(refs):
    """The reference over the concatenation of several batches."""
    out = {"loss_sum": sum(r["loss_sum"] for r in refs), "n": sum(r["n"] for r in refs),
           "n_correct": sum(r["n_correct"] for r in refs),
           "support": sum(r["support"] for r in refs), "hit": sum(r["hit"] for r in refs)}
    return out


def pack_block(loss_sum, n, n_correct, support, hit):
    """An accumulator block (CPU int64) from its parts: the layout include/fastvim_hip.h documents."""
    C = len(support)
    b = torch.zeros(3 + 2 * C, dtype=torch.int64)
    b[:1].view(torch.float64)[0] = float(loss_sum)
    b[1], b[2] = int(n), int(n_correct)
    b[3:3 + C] = torch.as_tensor(support, dtype=torch.int64)
    b[3 + C:] = torch.as_tensor(hit, dtype=torch.int64)
    return b


def unpack_block(block):
    b = block.detach().cpu().contiguous()
    C = (b.numel() - 3) // 2
    return {"loss_sum": float(b[:1].view(torch.float64)[0]), "n": int(b[1]), "n_correct": int(b[2]),
            "support": b[3:3 + C].clone(), "hit": b[3 + C:].clone()}
