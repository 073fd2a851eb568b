"""Plain torch reference of the channel-last scan launches (csrc/scan_cl.hip), in the kernels' own layouts.

    xc     (2, B, Lc, d_in)      the pooled conv output u, one copy per direction
    x_dbl  (2, B * Lc, R + 32)   [dt_low | B | C] per pooled row
    delta  = softplus(dt_low @ Wdt^T + bias),  A = -exp(A_log)
    h_t    = exp(delta_t A) h_{t-1} + delta_t B_t u_t,   y_t = <h_t, C_t>

Direction 0 walks the pooled rows in ascending, direction 1 in descending order.  ``scan`` runs the recurrence step by
step, vectorised over direction, batch element, channel and state, in the dtype it is given: float64 is the reference,
float32 the emulation ``test_scan_cl_ref_cpu.py`` holds to the same bounds as the kernels.  Gradients are autograd's.

The kernels' partial outputs come out of the same function by masking the output gradient (a channel's output depends
on no other channel's u or delta; a batch element's on no other element's inputs):

* the ``dx_dbl`` slice of channel chunk c is the x_dbl gradient with ``dyc`` zeroed outside the chunk's channels;
* the parameter gradient of ONE batch element is the gradient with ``dyc`` zeroed outside that element.  All of them
  are taken in one backward pass by giving every batch element its own copy of the parameters (``per_element``):
  the copy of element b receives exactly the masked gradient (``test_scan_cl_ref_cpu.py`` pins the two against each
  other).  A workgroup's partial row is the sum over its NBB elements; a segment-parallel launch writes S rows per
  element whose sum is the element's gradient.

The mutation switches of ``scan`` (``delta_scale``, ``dir1_ascending``, ``drop_rank``) exist for the CPU tests that show
a wrong kernel would be noticed; nothing else sets them.
"""
import torch
import torch.nn.functional as F

N = 16
F64 = torch.float64
SENTINEL = -16384.0              # exact in bf16 and fp32; no input or result comes near it

# the project's fp32 bounds (test_config34_gpu.py), each times max(1, max|ref|) OF THE PIECE compared
TOL_Y, TOL_STATE, TOL_DU, TOL_DXDBL, TOL_PARAM = 1e-5, 1e-5, 2e-5, 5e-5, 1e-4


def make_inputs(B, Lc, d_in, R, bf16, seed, dyc_per_direction=False, with_wx=False):
    """Seeded inputs (the recipe of test_config34_gpu._scan_cl_case).  bf16: xc and x_dbl are rounded to the storage type
    here, BEFORE any reference sees them -- the kernels read exactly these values."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    xc = rn(2, B, Lc, d_in)
    x_dbl = rn(2, B * Lc, R + 2 * N)
    x_dbl[..., :R] *= 0.5
    inp = dict(
        Wdt=rn(2, d_in, R) * R ** -0.5,
        bdt=torch.rand(2, d_in, generator=g) - 3.0,
        A_log=torch.log(torch.arange(1, N + 1, dtype=torch.float32)).repeat(2, d_in, 1) + 0.1 * rn(2, d_in, N),
        dyc=rn(2 if dyc_per_direction else 1, B, Lc, d_in))
    if with_wx:
        inp["Wx"] = rn(2, R + 2 * N, d_in) * d_in ** -0.5
        if bf16:
            inp["Wx"] = inp["Wx"].bfloat16().float()
    if bf16:
        xc, x_dbl = xc.bfloat16().float(), x_dbl.bfloat16().float()
    inp.update(xc=xc, x_dbl=x_dbl, B=B, Lc=Lc, d_in=d_in, R=R, bf16=bf16)
    return inp


def scan(xc, x_dbl, Wdt, bdt, A_log, delta_scale=1.0, dir1_ascending=False, drop_rank=None):
    """y (2, B, Lc, d_in) in row order, and the state after every step (2, B, Lc, d_in, N) in WALK order (detached):
    ``states[k, b, s]`` is direction k's state after its s-th step.  Parameters are (2, d_in, ...) or, with one copy per
    batch element, (2, B, d_in, ...).  Runs in the dtype of ``xc``."""
    _, B, Lc, d_in = xc.shape
    R = Wdt.shape[-1]
    xd = x_dbl.reshape(2, B, Lc, R + 2 * N)
    if not dir1_ascending:        # walk order: direction 1 reversed
        xc = torch.stack([xc[0], xc[1].flip(1)])
        xd = torch.stack([xd[0], xd[1].flip(1)])
    if Wdt.dim() == 3:
        Wdt, bdt, A_log = Wdt[:, None], bdt[:, None], A_log[:, None]
    if drop_rank is not None:
        Wdt = torch.cat([Wdt[..., :drop_rank], torch.zeros_like(Wdt[..., drop_rank:drop_rank + 1]), Wdt[..., drop_rank + 1:]], -1)
    delta = F.softplus(xd[..., :R] @ Wdt.transpose(-1, -2) + bdt[:, :, None]) * delta_scale              # (2, B, Lc, d_in)
    A = -torch.exp(A_log)                                                                                 # (2, 1 | B, d_in, N)
    Bm, Cm = xd[..., R:R + N], xd[..., R + N:]
    h = xc.new_zeros(2, B, d_in, N)
    ys, hs = [], []
    for t in range(Lc):
        dt = delta[:, :, t, :, None]
        h = torch.exp(dt * A) * h + dt * Bm[:, :, t, None, :] * xc[:, :, t, :, None]
        ys.append((h * Cm[:, :, t, None, :]).sum(-1))
        hs.append(h.detach())
    y = torch.stack(ys, 2)
    if not dir1_ascending:
        y = torch.stack([y[0], y[1].flip(1)])
    return y, torch.stack(hs, 2)


def checkpoints(states):
    """(2, B, nchunk, d_in, N): the state ENTERING each 16-step chunk -- chunk c >= 1 holds the state after walk step
    16 c - 1; slot 0 (the zero state entering the sequence, which no kernel stores) is zero here."""
    _, B, Lc, d_in, _ = states.shape
    nchunk = (Lc + 15) // 16
    ck = states.new_zeros(2, B, nchunk, d_in, N)
    for c in range(1, nchunk):
        ck[:, :, c] = states[:, :, 16 * c - 1]
    return ck


def param_rows(dA_log, dWdt, dbdt):
    """Per-element parameter gradients (2, B, d_in, .) -> the kernels' partial-row layout (B, 2 * d_in * (N + R + 1)):
    per direction [dA_log (d_in, N) | d Wdt (d_in, R) | d bias (d_in)]."""
    B = dA_log.shape[1]
    per_dir = torch.cat([dA_log.reshape(2, B, -1), dWdt.reshape(2, B, -1), dbdt.reshape(2, B, -1)], -1)      # (2, B, per_dir)
    return per_dir.transpose(0, 1).reshape(B, -1)


def reference(inp, dtype=F64, chunk_channels=None, dyc=None, per_element=True, **mutation):
    """Everything a launch is compared with, in ``dtype``: y, states, ckpt, du (2, B, Lc, d_in), dx_dbl (2, B * Lc, W),
    ``slices`` (nchunks, 2, B * Lc, W) for channel chunks of ``chunk_channels`` channels (None: no slices), ``rows``
    (B, 2 * d_in * (N + R + 1)) the per-element parameter gradients.  ``dyc``: overrides the case's output gradient."""
    B, Lc, d_in, R = inp["B"], inp["Lc"], inp["d_in"], inp["R"]
    c = lambda t: t.to(dtype).clone().requires_grad_()
    xc, xd = c(inp["xc"]), c(inp["x_dbl"])
    ex = (lambda t: t[:, None].expand(2, B, *t.shape[1:])) if per_element else (lambda t: t)
    W_, b_, Al = c(ex(inp["Wdt"])), c(ex(inp["bdt"])), c(ex(inp["A_log"]))
    y, states = scan(xc, xd, W_, b_, Al, **mutation)
    g = (inp["dyc"] if dyc is None else dyc).to(dtype).expand(2, B, Lc, d_in)
    du, dxd, dW, db, dAl = torch.autograd.grad(y, (xc, xd, W_, b_, Al), g, retain_graph=chunk_channels is not None)
    out = dict(y=y.detach(), states=states, ckpt=checkpoints(states), du=du, dx_dbl=dxd)
    out["rows"] = param_rows(dAl, dW, db) if per_element else torch.cat([dAl.reshape(2, -1), dW.reshape(2, -1), db.reshape(2, -1)], -1).reshape(1, -1)
    if chunk_channels is not None:
        sl = []
        for c0 in range(0, d_in, chunk_channels):
            m = torch.zeros(d_in, dtype=dtype)
            m[c0:c0 + chunk_channels] = 1
            sl.append(torch.autograd.grad(y, xd, g * m, retain_graph=True)[0])
        out["slices"] = torch.stack(sl)
    return out


def group_rows(rows, nbb):
    """Per-element rows (B, P) -> the rows of workgroups that walk ``nbb`` consecutive elements (B / nbb, P)."""
    return rows.reshape(rows.shape[0] // nbb, nbb, -1).sum(1)


def fused_xdbl_ref(xc, Wx):
    """The fused forward's x_proj product from the bf16 operands as stored, and the elementwise bound its bf16 result is
    held to: one storage rounding of the exact product, plus fp32 accumulation of d_in terms (the derived form of
    ``mixer_family_ref.fused_proj_ref``).  xc (2, B, Lc, d_in), Wx (2, W, d_in) -> (2, B * Lc, W) each."""
    d_in = xc.shape[-1]
    P = torch.einsum("kbld,kwd->kblw", xc.double(), Wx.double()).reshape(2, -1, Wx.shape[1])
    absP = torch.einsum("kbld,kwd->kblw", xc.double().abs(), Wx.double().abs()).reshape(2, -1, Wx.shape[1])
    return P, 2.0 ** -8 * P.abs() + d_in * 2.0 ** -24 * absP


# ------------------------------------------------------------------------------------------------ comparisons
def worst_ratio(got, ref, tol, piece_dims):
    """max over pieces of max|got - ref| / (tol * max(1, max|ref| of the piece)); a piece is one index of the leading
    ``piece_dims`` dimensions.  <= 1 passes."""
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    n = 1
    for s in ref.shape[:piece_dims]:
        n *= s
    e = (got - ref).abs().reshape(n, -1).amax(1)
    s = ref.abs().reshape(n, -1).amax(1).clamp_min(1.0)
    return (e / (tol * s)).max().item()


class Report:
    """Collects err / bound ratios per tensor; ``check`` raises listing every tensor above 1."""

    def __init__(self):
        self.ratios = {}

    def add(self, name, got, ref, tol, piece_dims):
        r = worst_ratio(got, ref, tol, piece_dims)
        self.ratios[name] = max(r, self.ratios.get(name, 0.0))
        return r

    def add_elementwise(self, name, got, ref, bound):
        r = ((got.double().cpu() - ref.double().cpu()).abs() / bound).max().item()
        self.ratios[name] = max(r, self.ratios.get(name, 0.0))
        return r

    def bad(self):
        return {k: v for k, v in self.ratios.items() if not v <= 1.0}

    def check(self, what=""):
        assert not self.bad(), (what, self.bad())


def compare_forward(rep, y, ref, ckpt=None):
    """y (2, B, Lc, d_in) per (direction, element); checkpoints (2, B, nchunk, d_in, N), chunks 1.. only, likewise."""
    rep.add("y", y, ref["y"], TOL_Y, 2)
    if ckpt is not None and ckpt.shape[2] > 1:
        rep.add("ckpt", ckpt[:, :, 1:], ref["ckpt"][:, :, 1:], TOL_STATE, 2)


def compare_backward(rep, dxc, slices, rows, ref, nbb=1, segments=1):
    """du per (direction, element); every dx_dbl chunk slice on its own; every partial row on its own -- with segments the
    sum of an element's S rows against that element's gradient (rows are (element, segment) ordered: row b S + s; the
    batch-2 segment cases tell that from (segment, element))."""
    rep.add("du", dxc, ref["du"], TOL_DU, 2)
    rep.add("dx_dbl", slices, ref["slices"], TOL_DXDBL, 1)
    if segments > 1:
        rows = rows.double().cpu().reshape(-1, segments, rows.shape[-1]).sum(1)
    rep.add("rows", rows, group_rows(ref["rows"], nbb), TOL_PARAM, 1)
