"""Float64 references of the fused mixer's four row-kernel families, in the kernels' own layouts.

Plain helpers (no fixtures, nothing here imports ``fastvim_amd``) shared by ``test_mixer_family_ref_cpu.py`` (which pins
them to ``oracle.fastvim_mixer_oracle``) and ``test_mixer_families_gpu.py`` (which holds the HIP kernels to them).
Everything is plain torch on the CPU in float64, built on ``oracle.causal_conv1d_oracle`` and
``torch.nn.functional.layer_norm``; every gradient is autograd's.

Layouts (include/fastvim_hip.h):

* ``x`` / ``z``     (B, L, d_in): the two halves of ``xz`` (B, L, 2*d_in), MEMORY token order;
* token geometry   sequence position ``s = (i*cols + j)*tpp + c`` (pooling row i, patch column j, channel token c) is
  memory token ``(i*s_i + j*s_j)*tpp + c`` with ``(s_i, s_j) = (cols, 1)`` (natural) or ``(1, rows)`` (transposed);
* pooled tensors   (2, B, rows*tpp, d_in), ``[0]`` forward / ``[1]`` backward direction, pooled index ``i*tpp + c``
  in original order;
* partial row      ``[dw (d_in*4) | dw_b (d_in*4) | db | db_b | dD | dD_b]`` (12*d_in), ``[d ln_w | d ln_b]`` (2, d_in).

The 0.5 factors (csrc/mixer_bwd.hip): ``o = 0.5*(expand(yc_f + yc_b) + skip)``; combine's adjoint hands on
``d_o = dL/do`` unhalved and ``dyc = 0.5 * sum over cols of d_o`` (one tensor, the gradient of EITHER direction's scan
output); the conv + pool adjoint folds the remaining 0.5 into D: it differentiates
``L = <d_o, 0.5*skip(x)> + <dxc + dxc2, xc(x)>``.
"""
import torch
import torch.nn.functional as F

from oracle import causal_conv1d_oracle

F64 = torch.float64


def seq_to_mem(rows, cols, tpp=1, transposed=False):
    """(L,) long: memory token of every sequence position."""
    s_i, s_j = (1, rows) if transposed else (cols, 1)
    i = torch.arange(rows).view(rows, 1, 1)
    j = torch.arange(cols).view(1, cols, 1)
    c = torch.arange(tpp).view(1, 1, tpp)
    return ((i * s_i + j * s_j) * tpp + c).reshape(-1)


def pooled_index_of_mem(rows, cols, tpp=1, transposed=False):
    """(L,) long: pooled index ``i*tpp + c`` of every MEMORY token."""
    i = torch.arange(rows).view(rows, 1, 1)
    c = torch.arange(tpp).view(1, 1, tpp)
    grp = (i * tpp + c).expand(rows, cols, tpp).reshape(-1)           # by sequence position
    out = torch.empty_like(grp)
    out[seq_to_mem(rows, cols, tpp, transposed)] = grp
    return out


def _to_mem(t_bdl, perm):
    """(B, d, L) in sequence order -> (B, L, d) in memory order."""
    out = torch.empty_like(t_bdl.permute(0, 2, 1))
    return out.index_copy(1, perm, t_bdl.permute(0, 2, 1))


def _convs(x, w_f, b_f, w_b, b_b, perm):
    xs = x[:, perm].permute(0, 2, 1)                                   # (B, d_in, L), sequence order
    cf = causal_conv1d_oracle(xs, w_f, b_f, "silu", compute_dtype=F64, out_dtype=F64)
    cb = causal_conv1d_oracle(xs, w_b, b_b, "silu", anticausal=True, compute_dtype=F64, out_dtype=F64)
    return cf, cb


def _pool(conv, rows, cols, tpp, pool_max, scaling, amax=None):
    """conv (B, d, L) sequence order -> pooled (B, rows*tpp, d), argmax columns (same shape, float64) or None.
    ``amax`` given (max pooling): the pooled value is taken AT that column (the adjoint's definition)."""
    Bsz, d, _ = conv.shape
    grid = conv.reshape(Bsz, d, rows, cols, tpp)
    if not pool_max:
        return (scaling * grid.mean(3)).reshape(Bsz, d, rows * tpp).permute(0, 2, 1), None
    if amax is None:
        val, idx = grid.max(3)
    else:
        idx = amax.permute(0, 2, 1).reshape(Bsz, d, rows, tpp).long()
        val = grid.gather(3, idx.unsqueeze(3)).squeeze(3)
    return val.reshape(Bsz, d, rows * tpp).permute(0, 2, 1), idx.reshape(Bsz, d, rows * tpp).permute(0, 2, 1).to(F64)


def conv_pool_ref(x, w_f, b_f, w_b, b_b, D, D_b, rows, cols, tpp=1, pool_max=False, scaling=1.0, transposed=False,
                  amax=None):
    """Both depthwise convs + SiLU along the sequence, pooling over ``cols``, the D-weighted skip.

    x (B, L, d_in) memory order; w_* (d_in, 4); b_* (d_in) or None; D, D_b (d_in) or None (then ``skip`` is None).
    Returns conv_f, conv_b, skip (B, L, d_in) memory order, xc (2, B, rows*tpp, d_in) and argmax (like xc; None for
    mean pooling).  Mean pooling is ``scaling * mean over cols``, max pooling ``.max`` over cols (``scaling`` unused).
    ``amax`` (like xc): pool at these columns instead of the maxima."""
    perm = seq_to_mem(rows, cols, tpp, transposed)
    cf, cb = _convs(x.to(F64), w_f.to(F64), None if b_f is None else b_f.to(F64), w_b.to(F64),
                    None if b_b is None else b_b.to(F64), perm)
    pf, af = _pool(cf, rows, cols, tpp, pool_max, scaling, None if amax is None else amax[0])
    pb, ab = _pool(cb, rows, cols, tpp, pool_max, scaling, None if amax is None else amax[1])
    xc = torch.stack([pf, pb])
    arg = torch.stack([af, ab]) if pool_max else None
    conv_f, conv_b = _to_mem(cf, perm), _to_mem(cb, perm)
    skip = None if D is None else D.to(F64) * conv_f + D_b.to(F64) * conv_b
    return conv_f, conv_b, xc, skip, arg


def combine_ref(z, skip, yc, ln_w, ln_b, eps, rows, cols, tpp=1, transposed=False):
    """o = 0.5*(expand(yc_f + yc_b) + skip); g = LN(o) * silu(z) (without ``ln_w``: g = o * silu(z)).
    z, skip (B, L, d_in) memory order; yc (2, B, rows*tpp, d_in).  Returns o, g (B, L, d_in), mean, rstd (B*L) (None
    without the norm)."""
    grp = pooled_index_of_mem(rows, cols, tpp, transposed)
    z, skip, yc = z.to(F64), skip.to(F64), yc.to(F64)
    o = 0.5 * ((yc[0] + yc[1])[:, grp] + skip)
    d_in = o.shape[-1]
    if ln_w is None:
        return o, o * F.silu(z), None, None
    g = F.layer_norm(o, (d_in,), ln_w.to(F64), ln_b.to(F64), eps) * F.silu(z)
    mean = o.mean(-1)
    rstd = torch.rsqrt(o.var(-1, unbiased=False) + eps)
    return o, g, mean.reshape(-1), rstd.reshape(-1)


def combine_adjoint_ref(dg, z, skip, yc, ln_w, ln_b, eps, rows, cols, tpp=1, transposed=False):
    """Adjoint of ``combine_ref`` for the cotangent ``dg`` of g: returns dz, d_o = dL/do (B, L, d_in), dyc
    (B, rows*tpp, d_in) = 0.5 * sum over cols of d_o (autograd's gradient of yc_f, which equals that of yc_b) and
    d ln_w, d ln_b (None without the norm)."""
    z = z.detach().to(F64).requires_grad_()
    yc = yc.detach().to(F64).requires_grad_()
    lw = None if ln_w is None else ln_w.detach().to(F64).requires_grad_()
    lb = None if ln_b is None else ln_b.detach().to(F64).requires_grad_()
    grp = pooled_index_of_mem(rows, cols, tpp, transposed)
    o = 0.5 * ((yc[0] + yc[1])[:, grp] + skip.detach().to(F64))
    o.retain_grad()
    d_in = o.shape[-1]
    h = o if lw is None else F.layer_norm(o, (d_in,), lw, lb, eps)
    g = h * F.silu(z)
    (g * dg.to(F64)).sum().backward()
    assert torch.equal(yc.grad[0], yc.grad[1])
    return (z.grad, o.grad, yc.grad[0], None if lw is None else lw.grad, None if lb is None else lb.grad)


def conv_pool_adjoint_ref(x, w_f, b_f, w_b, b_b, D, D_b, d_o, dxc, rows, cols, tpp=1, pool_max=False, scaling=1.0,
                          transposed=False, amax=None, dxc2=None):
    """Gradients of ``L = <d_o, 0.5*skip(x)> + <dxc + dxc2, xc(x)>``: dx (B, L, d_in) memory order and the partial row
    ``[dw | dw_b | db | db_b | dD | dD_b]`` (12*d_in; the bias segments are those of a zero bias where one is absent).
    Max pooling needs ``amax`` (like xc): the pooled gradient goes to that column only."""
    assert not pool_max or amax is not None
    d_in = x.shape[-1]
    leaf = lambda t: t.detach().to(F64).clone().requires_grad_()
    x, w_f, w_b, D, D_b = leaf(x), leaf(w_f), leaf(w_b), leaf(D), leaf(D_b)
    b_f = leaf(torch.zeros(d_in) if b_f is None else b_f)
    b_b = leaf(torch.zeros(d_in) if b_b is None else b_b)
    _, _, xc, skip, _ = conv_pool_ref(x, w_f, b_f, w_b, b_b, D, D_b, rows, cols, tpp, pool_max, scaling, transposed,
                                      amax=amax if pool_max else None)
    dtot = dxc.to(F64) if dxc2 is None else dxc.to(F64) + dxc2.to(F64)
    ((d_o.to(F64) * 0.5 * skip).sum() + (dtot * xc).sum()).backward()
    part = torch.cat([w_f.grad.reshape(-1), w_b.grad.reshape(-1), b_f.grad, b_b.grad, D.grad, D_b.grad])
    return x.grad, part


# ------------------------------------------------------------------------------------------------ bounds
def cpu64(t):
    return None if t is None else t.detach().double().cpu()


def close(errs, name, got, ref, tol, stored_bf16=False, elementwise_scale=False):
    """Record a violation of |got - ref| <= tol * max(1, max|ref|) (elementwise max(1, |ref|) for the LayerNorm
    statistics), plus one bf16 storage rounding 2**-8 * |ref| where the kernel stores the tensor in bf16."""
    got, ref = cpu64(got), ref.detach().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    bound = tol * (ref.abs().clamp_min(1.0) if elementwise_scale else max(1.0, ref.abs().max().item()))
    if stored_bf16:
        bound = 2.0 ** -8 * ref.abs() + bound
    err = (got - ref).abs()
    worst = (err - bound).argmax()
    print(f"{name}: max err {err.max().item():.3e}  max|ref| {ref.abs().max().item():.3e}  "
          f"worst err/bound {(err / bound).max().item():.3f}")
    if not bool((err <= bound).all()) or not bool(torch.isfinite(got).all()):
        errs.append((name, err.reshape(-1)[worst].item(), tuple(int(k) for k in torch.unravel_index(worst, err.shape))))
