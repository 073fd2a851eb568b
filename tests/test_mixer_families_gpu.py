"""The fused mixer's four row-kernel families, each on its own against the float64 references of
``mixer_family_ref.py``: ``fv_mixer_conv_pool_fwd``, ``fv_mixer_combine_fwd``, ``fv_mixer_combine_bwd`` and
``fv_mixer_conv_pool_bwd(2)`` through ``fastvim_amd.mixer_ops``.

CASES is tied to the dispatcher: every case states, per family, the launch plan it is there for (form, channels per
lane, channel slabs or not; ``tokens_per_patch`` > 1, the pooling mode and the storage type are the case's own), and
every test first asserts through ``fv_mixer_plan`` that its shape still takes that plan.
``test_mixer_family_ref_cpu.py`` sweeps ``fv_mixer_plan`` and asserts that every distinct supported plan key occurs here.

A case is a chain conv+pool forward -> combine forward -> combine adjoint -> conv+pool adjoint.  Each kernel's
reference is computed from the inputs AS THAT KERNEL SEES THEM: the storage-rounded ``xz``, and the tensors the previous
kernel of the chain actually wrote (``skip``, ``mean`` / ``rstd``, ``d_o``, the argmax columns) -- so every comparison
isolates one launch, and the adjoint of max pooling is exactly defined (the gradient goes to the column the forward
stored; nothing is excused there).

Every launch runs twice into freshly allocated buffers that are prefilled with a sentinel and one row (``d_inner``
elements) longer than the kernel needs: the two results must be bit-identical (no atomics), an element the kernel
leaves unwritten shows as the sentinel, and the slack row must still hold the sentinel afterwards.

Tolerances -- none measured from the kernels.  fp32 storage: the bounds ``test_config34_gpu.py`` and
``test_mixer_gpu.py`` hold the fp32 kernels to, per tensor, times ``max(1, max|ref|)``: per-token tensors 1e-5 forward
(xc, skip, g), 2e-5 backward (dz, d_o, dx); sums over one pooling row (dyc) 5e-5; sums over all tokens (the eight
parameter gradients) 1e-4; mean / rstd ``1e-5 * max(1, |ref|)`` elementwise.  bf16 storage: a tensor the kernel stores
in bf16 gets one storage rounding on top, elementwise ``|got - ref| <= 2**-8 * |ref| + fp32 bound``
(``test_scan_gpu.py``'s form); the fp32 outputs of a bf16 launch (dyc, mean, rstd, the partial rows) keep the fp32
bounds.

Max pooling: the forward's argmax columns must equal the float64 argmax except in groups whose float64 top two values
lie closer than ``1e-5 * max(1, |top|)`` (the kernel compares in fp32); such groups stay at or below 0.5 % of a case.
The seeds of the max-pooling cases were checked on the CPU to satisfy that on the reference alone
(``test_mixer_family_ref_cpu.py::test_max_pool_seeds_have_few_near_ties``).  The pooled value is compared everywhere.
"""
import ctypes
import math

import pytest
import torch

import mixer_family_ref as R

F64 = torch.float64
CONV_FWD, COMB_FWD, COMB_BWD, CONV_BWD = 0, 1, 2, 3
FAMILIES = {"CF": CONV_FWD, "MF": COMB_FWD, "MB": COMB_BWD, "CB": CONV_BWD}
FORMS = {"G": 1, "R": 2, "C": 3, "W": 4}        # generic, whole-row, cell walker, wave per token
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
SENTINEL = -16384.0                              # exact in bf16
BF16_HALF_ULP = 2.0 ** -8


def _case(name, d, rows, cols, plans, tpp=1, B=2, pm=0, dt="f32", tr=False, opts=(), seed=0):
    """plans: "CF:G1 MF:G1 MB:G1 CB:G2s" -- family:form, channels per lane, "s" = more than one channel slab.  A family
    that is not named is not launched (the shape has no plan there, or the case is forward only)."""
    pl = {}
    for tok in plans.split():
        fam, spec = tok.split(":")
        slabs = spec.endswith("s")
        spec = spec[:-1] if slabs else spec
        pl[FAMILIES[fam]] = (FORMS[spec[0]], int(spec[1:]), slabs)
    return dict(name=name, d=d, rows=rows, cols=cols, tpp=tpp, B=B, pm=pm, dt=dt, tr=tr, opts=frozenset(opts), plans=pl, seed=seed)


ALL_G1 = "CF:G1 MF:G1 MB:G1 CB:G1"
CASES = [
    # ---- ragged channels (d_inner no multiple of 64: the `act` lanes), one channel per lane, all four families
    _case("d40_3x3_b3_f32", 40, 3, 3, ALL_G1, B=3),                       # 9 pooling rows on 4 row groups: row-group tail
    _case("d40_2x5_max_bf16_t", 40, 2, 5, ALL_G1, pm=1, dt="bf16", tr=True),
    _case("d40_1x3_bf16", 40, 1, 3, ALL_G1, dt="bf16"),                   # rows = 1: no row above or below
    _case("d96_3x3_bf16_noln", 96, 3, 3, ALL_G1, dt="bf16", opts=("noln",)),
    _case("d96_2x4_f32_t", 96, 2, 4, ALL_G1, tr=True, opts=("nobias", "scale")),
    _case("d40_2x3_tpp2_f32", 40, 2, 3, ALL_G1, tpp=2),                    # LDS slot accumulators, one channel per lane
    _case("d40_2x3_tpp2_max_bf16", 40, 2, 3, ALL_G1, tpp=2, pm=1, dt="bf16"),
    # ---- d_inner 64: generic, persistent grids (second and later iterations, ragged last one)
    _case("d64_3x3_b701_f32", 64, 3, 3, ALL_G1, B=701, opts=("persistent",)),
    _case("d64_1x255_max_bf16", 64, 1, 255, ALL_G1, pm=1, dt="bf16", opts=("argmax_exact",)),
    _case("d64_5x1_f32_fwd", 64, 5, 1, "CF:G1 MF:G1", opts=("short",)),    # conv window spans four pooling rows
    _case("d64_5x2_max_bf16_fwd", 64, 5, 2, "CF:G1 MF:G1", pm=1, dt="bf16", opts=("short",)),
    _case("d64_4x2_f32_t_fwd", 64, 4, 2, "CF:G1 MF:G1", tr=True, opts=("short",)),
    _case("d64_1x2_f32_fwd", 64, 1, 2, "CF:G1 MF:G1", opts=("short",)),    # the whole sequence is shorter than the window
    _case("d64_1x1_b3_bf16_fwd", 64, 1, 1, "CF:G1 MF:G1", B=3, dt="bf16", opts=("short",)),
    # ---- kernel instantiations the plan does not name: 7-token forward tiles (cols a multiple of 7), 8-token fetch
    # groups of the streaming adjoint (cols > 14), row-group tails of the whole-row / cell-walking adjoints
    _case("d64_2x15_f32", 64, 2, 15, ALL_G1),
    _case("d128_3x14_b3_max_f32", 128, 3, 14, "CF:G1 MF:G2 MB:G1 CB:G2", B=3, pm=1),
    _case("d128_3x14_b3_bf16", 128, 3, 14, "CF:R2 MF:G2 MB:G1 CB:R2", B=3, dt="bf16"),
    _case("d128_3x24_b3_f32", 128, 3, 24, "CF:C2 MF:G2 MB:G1 CB:C2", B=3),
    _case("d128_3x2_tpp8_b3_bf16", 128, 3, 2, "CF:C2 MF:G2 MB:G2 CB:C2", tpp=8, B=3, dt="bf16"),
    _case("d384_1x3_b1_bf16", 384, 1, 3, "CF:G6 MF:W6 MB:W6 CB:G2", B=1, dt="bf16"),
    # ---- d_inner 128: channel pairs
    _case("d128_2x3_f32", 128, 2, 3, "CF:G1 MF:G2 MB:G1 CB:G2"),
    _case("d128_2x5_max_bf16_t", 128, 2, 5, "CF:G1 MF:G2 MB:G1 CB:G2", pm=1, dt="bf16", tr=True),
    _case("d128_2x3_tpp2_f32", 128, 2, 3, "CF:G2 MF:G2 MB:G2 CB:G2", tpp=2),
    _case("d128_2x3_tpp2_max_bf16_t", 128, 2, 3, "CF:G2 MF:G2 MB:G2 CB:G2", tpp=2, pm=1, dt="bf16", tr=True),
    _case("d128_2x2_tpp8_bf16", 128, 2, 2, "CF:C2 MF:G2 MB:G2 CB:C2", tpp=8, dt="bf16"),        # cell walkers, tpp 8
    _case("d128_3x2_tpp8_f32_t", 128, 3, 2, "CF:C2 MF:G2 MB:G2 CB:C2", tpp=8, tr=True),
    _case("d128_2x14_f32_dxc2", 128, 2, 14, "CF:R2 MF:G2 MB:G1 CB:R2", opts=("dxc2",)),          # whole-row kernels
    _case("d128_1x16_bf16_t", 128, 1, 16, "CF:R2 MF:G2 MB:G1 CB:R2", dt="bf16", tr=True),
    _case("d128_1x24_bf16", 128, 1, 24, "CF:C2 MF:G2 MB:G1 CB:C2", dt="bf16"),                   # dense long rows, rows = 1
    _case("d128_2x32_f32_t", 128, 2, 32, "CF:C2 MF:G2 MB:G1 CB:C2", tr=True, opts=("scale",)),
    # ---- d_inner 256: four channels per lane; the whole-row adjoint's block split depends on the storage type
    _case("d256_3x3_f32_offset", 256, 3, 3, "CF:G4 MF:G4 MB:G4 CB:G2", opts=("offset",)),
    _case("d256_2x4_max_bf16", 256, 2, 4, "CF:G4 MF:G4 MB:G4 CB:G2", pm=1, dt="bf16"),
    _case("d256_2x3_tpp2_bf16", 256, 2, 3, "CF:G2 MF:G4 MB:G2 CB:G2", tpp=2, dt="bf16"),
    _case("d256_2x14_f32", 256, 2, 14, "CF:R2 MF:G4 MB:G4 CB:R2", opts=("scale",)),
    _case("d256_2x14_bf16_dxc2", 256, 2, 14, "CF:R2 MF:G4 MB:G4 CB:R2s", dt="bf16", opts=("dxc2",)),
    # ---- d_inner 384: six channels per lane, wave-per-token combine
    _case("d384_3x3_b3_f32_offset", 384, 3, 3, "CF:G6 MF:W6 MB:W6 CB:G2", B=3, opts=("offset",)),   # 9 groups on WAVE_NW 4
    _case("d384_2x5_max_bf16_t", 384, 2, 5, "CF:G6 MF:W6 MB:W6 CB:G2", pm=1, dt="bf16", tr=True),
    _case("d384_3x3_b701_bf16", 384, 3, 3, "CF:G6 MF:W6 MB:W6 CB:G2", B=701, dt="bf16", opts=("persistent",)),
    _case("d384_2x2_tpp8_f32", 384, 2, 2, "CF:C2s MF:W6 MB:W6 CB:C2s", tpp=8),
    _case("d384_2x24_f32", 384, 2, 24, "CF:C2s MF:W6 MB:W6 CB:C2s"),
    _case("d384_2x14_f32_dxc2_noD", 384, 2, 14, "CF:R2 MF:W6 MB:W6 CB:R2s", opts=("dxc2", "noD")),
    _case("d384_2x14_bf16_dxc2_t", 384, 2, 14, "CF:R2 MF:W6 MB:W6 CB:R2", dt="bf16", tr=True, opts=("dxc2",)),
    _case("d384_2x16_bf16", 384, 2, 16, "CF:R2 MF:W6 MB:W6 CB:R2s", dt="bf16", opts=("nobias",)),
    # ---- wider
    _case("d640_2x14_bf16", 640, 2, 14, "CF:R2s MF:G2 MB:G1 CB:R2s", dt="bf16"),
    _case("d768_2x3_bf16_noln", 768, 2, 3, "CF:G6 MF:W12 MB:W12 CB:G2", dt="bf16", opts=("noln",)),
    _case("d768_2x3_tpp2_f32_t", 768, 2, 3, "CF:G2 MF:W12 MB:W12 CB:G2", tpp=2, tr=True),
    _case("d1088_2x3_f32_fwd", 1088, 2, 3, "CF:G1s"),                       # 17 waves of single channels: forward only
    _case("d1088_2x3_max_bf16_fwd", 1088, 2, 3, "CF:G1s", pm=1, dt="bf16"),
    _case("d1088_2x3_tpp2_bf16_fwd", 1088, 2, 3, "CF:G1s", tpp=2, dt="bf16"),
    _case("d1088_2x3_tpp2_max_f32_fwd", 1088, 2, 3, "CF:G1s", tpp=2, pm=1),
    _case("d1280_2x3_tpp2_f32", 1280, 2, 3, "CF:G4 MF:G4 MB:G4 CB:G2", tpp=2),
    _case("d1280_2x3_tpp2_max_bf16", 1280, 2, 3, "CF:G4 MF:G4 MB:G4 CB:G2", tpp=2, pm=1, dt="bf16"),
    _case("d1536_2x3_f32", 1536, 2, 3, "CF:G6 MF:W24 MB:W24 CB:G2"),
    _case("d1536_2x2_tpp2_bf16", 1536, 2, 2, "CF:G4 MF:W24 MB:W24 CB:G2", tpp=2, dt="bf16"),
    _case("d2048_2x3_f32", 2048, 2, 3, "CF:G4 MF:G4 MB:G4 CB:G2s"),
    _case("d2048_2x3_max_bf16_t", 2048, 2, 3, "CF:G4 MF:G4 MB:G4 CB:G2s", pm=1, dt="bf16", tr=True),
    _case("d2048_2x2_tpp2_f32", 2048, 2, 2, "CF:G4 MF:G4 MB:G4 CB:G2s", tpp=2),
    _case("d2048_2x2_tpp2_max_bf16", 2048, 2, 2, "CF:G4 MF:G4 MB:G4 CB:G2s", tpp=2, pm=1, dt="bf16"),
    _case("d2560_2x3_bf16_offset", 2560, 2, 3, "CF:G4s MF:G8 MB:G8 CB:G2s", dt="bf16", opts=("offset",)),
    _case("d2560_2x3_max_f32_t", 2560, 2, 3, "CF:G4s MF:G8 MB:G8 CB:G2s", pm=1, tr=True),
    _case("d2560_3x1_tpp3_f32", 2560, 3, 1, "CF:G1s MF:G8 MB:G8 CB:G2s", tpp=3),   # un-pooled rows x 1 x t, 8 channels per lane
    _case("d3072_2x3_f32", 3072, 2, 3, "CF:G6 MF:G6 MB:G6 CB:G2s"),
    _case("d3072_2x3_tpp2_bf16", 3072, 2, 3, "CF:G1s MF:G6 CB:G2s", tpp=2, dt="bf16"),      # no combine adjoint at this shape
    # ---- rows = 1 in the packed-math forms that have none above
    _case("d128_1x14_f32", 128, 1, 14, "CF:R2 MF:G2 MB:G1 CB:R2", opts=("dxc2",)),
    _case("d128_1x2_tpp8_f32", 128, 1, 2, "CF:C2 MF:G2 MB:G2 CB:C2", tpp=8),
]
for _i, _c in enumerate(CASES):
    _c["seed"] = 1000 + _i          # the seeds test_max_pool_seeds_have_few_near_ties checked
CASE_BY_NAME = {c["name"]: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


# ------------------------------------------------------------------------------------------------ plans (host only)
def query_plan(lib, family, B, rows, cols, tpp, d, pm, dt):
    out = (ctypes.c_int * 8)()
    i = ctypes.c_int
    rc = lib.fv_mixer_plan(i(family), i(B), i(rows), i(cols), i(tpp), i(d), i(pm), i(0 if dt == "f32" else 1), out)
    assert rc == 0
    return tuple(out)[:7]          # form, vec, waves, slabs, row_groups, lds_bytes, takes_dxc2


def plan_key(lib, family, rows, cols, tpp, d, pm, dt, B=2):
    """(family, form, vec, slabs > 1, tpp > 1, pool_max, dtype) of a shape, or None where it has no plan.  The pooling
    mode is part of the key for the conv + pool families only (the combine launches take none); the dtype is, where
    the two storage types' (form, vec, slabs > 1) differ at this shape, and None otherwise."""
    short = lambda p: (p[0], p[1], p[3] > 1)
    p = {t: short(query_plan(lib, family, B, rows, cols, tpp, d, pm, t)) for t in ("f32", "bf16")}
    if p[dt][0] == 0:
        return None
    return (family,) + p[dt] + (tpp > 1, pm if family in (CONV_FWD, CONV_BWD) else None, dt if p["f32"] != p["bf16"] else None)


def stated_key(lib, c, family):
    """The key a case CLAIMS for a family: its stated (form, vec, slabs) with the case's own tpp, pooling and dtype."""
    k = plan_key(lib, family, c["rows"], c["cols"], c["tpp"], c["d"], c["pm"], c["dt"], c["B"])
    return None if k is None else (family,) + c["plans"][family] + k[4:]


def assert_plan(lib, c, family):
    got = query_plan(lib, family, c["B"], c["rows"], c["cols"], c["tpp"], c["d"], c["pm"], c["dt"])
    assert (got[0], got[1], got[3] > 1) == c["plans"][family], (c["name"], family, got)
    return got


# ------------------------------------------------------------------------------------------------ inputs
def make_inputs(c):
    """Seeded CPU inputs of a case."""
    g = torch.Generator().manual_seed(c["seed"])
    rn = lambda *s: torch.randn(*s, generator=g)
    d, B, tpp = c["d"], c["B"], c["tpp"]
    Ltok, Lc = c["rows"] * c["cols"] * tpp, c["rows"] * tpp
    dt = DT[c["dt"]]
    o = c["opts"]
    inp = dict(
        xz=rn(B, Ltok, 2 * d).to(dt),
        cw=0.5 * rn(d, 4), cwb=0.5 * rn(d, 4),
        # nn.Conv1d's bias init for a depthwise width-4 conv is U(-1/2, 1/2); the mixer tests add 0.1 * randn to it
        cb=None if "nobias" in o else torch.rand(d, generator=g) - 0.5 + 0.1 * rn(d),
        cbb=None if "nobias" in o else torch.rand(d, generator=g) - 0.5 + 0.1 * rn(d),
        D=1 + 0.1 * rn(d), Db=1 + 0.1 * rn(d),
        ln_w=None if "noln" in o else 1 + 0.1 * rn(d), ln_b=None if "noln" in o else 0.1 * rn(d),
        yc=rn(2, B, Lc, d), dg=rn(B, Ltok, d).to(dt), dxc=rn(2, B, Lc, d),
        dxc2=rn(2, B, Lc, d).to(dt) if "dxc2" in o else None,
        scaling=0.25 if "scale" in o else 1.0, eps=1e-5)
    if "offset" in o:
        # every pre-norm row o = 0.5 * (yc_f + yc_b + skip) carries a common offset of at least 30 of its standard
        # deviations (where a one-pass variance would cancel): yc_f of a pooling group is raised, in all channels alike
        # (which leaves the row's deviation as it is), by 2 * 30 * the largest deviation among the group's tokens -- 2 %
        # on top for the storage rounding of the skip the kernel will read
        x = inp["xz"][..., :d]
        skip = R.conv_pool_ref(x, inp["cw"], inp["cb"], inp["cwb"], inp["cbb"], inp["D"], inp["Db"], c["rows"], c["cols"],
                               tpp, c["pm"], inp["scaling"], c["tr"])[3]
        grp = R.pooled_index_of_mem(c["rows"], c["cols"], tpp, c["tr"])
        std = (0.5 * ((inp["yc"][0] + inp["yc"][1]).double()[:, grp] + skip)).std(-1)                   # (B, L)
        worst = torch.zeros(B, Lc, dtype=F64).scatter_reduce(1, grp.expand(B, -1), std, "amax")
        inp["yc"][0] += (2 * 30 * 1.02 * worst).float()[..., None]
    return inp


def near_tie_groups(conv_mem, c):
    """Pooling groups of a max-pooled conv output (B, L, d) memory order whose float64 top two values lie closer than
    1e-5 * max(1, |top|): (2..., B, rows*tpp, d) bool like the pooled tensors."""
    perm = R.seq_to_mem(c["rows"], c["cols"], c["tpp"], c["tr"])
    Bsz, _, d = conv_mem.shape
    grid = conv_mem[:, perm].reshape(Bsz, c["rows"], c["cols"], c["tpp"], d)
    if c["cols"] == 1:
        return torch.zeros(Bsz, c["rows"] * c["tpp"], d, dtype=torch.bool)
    top = grid.topk(2, dim=2).values
    tie = (top[:, :, 0] - top[:, :, 1]) < 1e-5 * top[:, :, 0].abs().clamp_min(1.0)
    return tie.reshape(Bsz, c["rows"] * c["tpp"], d)


# ------------------------------------------------------------------------------------------------ GPU side
pytestmark = pytest.mark.gpu


class _PaddedTorch:
    """Stands in for the ``torch`` module inside ``fastvim_amd.mixer_ops`` while a kernel is launched: ``empty`` /
    ``empty_like`` hand out buffers that are one row (last dimension) longer than asked for and filled with SENTINEL."""

    def __init__(self):
        self.slack = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *shape, **kw):
        if len(shape) == 1 and not isinstance(shape[0], int):
            shape = tuple(shape[0])
        n = math.prod(shape)
        flat = torch.full((n + shape[-1],), SENTINEL, **kw)
        self.slack.append(flat[n:])
        return flat[:n].view(shape)

    def empty_like(self, t):
        return self.empty(*t.shape, device=t.device, dtype=t.dtype)

    def intact(self):
        return all(bool((s == SENTINEL).all()) for s in self.slack)


def _twice(fn):
    """Run a launch twice under the padded allocator; returns (outputs of the first run, bit-identical?, slack intact?)."""
    from fastvim_amd import mixer_ops as M
    pt = _PaddedTorch()
    M.torch = pt
    try:
        a, b = fn(), fn()
        torch.cuda.synchronize()
    finally:
        M.torch = torch
    flat = lambda r: [t for t in (r if isinstance(r, tuple) else (r,)) if t is not None]
    same = all(torch.equal(x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32),
                           y.view(torch.int16 if y.dtype == torch.bfloat16 else torch.int32)) for x, y in zip(flat(a), flat(b)))
    return a, same, pt.intact()


class Chain:
    """The launches of one case, each made once per session and kept on the CPU."""

    def __init__(self, c):
        self.c = c
        self.inp = make_inputs(c)
        self.dev = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in self.inp.items()}
        self.out = {}

    def _geo(self):
        c = self.c
        return c["rows"], c["cols"], c["tr"]

    def conv_fwd(self):
        if "conv_fwd" not in self.out:
            from fastvim_amd import mixer_ops as M
            c, v = self.c, self.dev
            rows, cols, tr = self._geo()
            call = lambda D, Db: M.conv_pool_fwd(v["xz"], v["cw"], v["cb"], v["cwb"], v["cbb"], rows, cols, tr, c["pm"],
                                                 v["scaling"], c["tpp"], D=D, D_b=Db)
            r, same, intact = _twice(lambda: call(v["D"], v["Db"]))
            xc, skip = r[0], r[1]
            res = dict(xc=xc, skip=skip, amax=r[2] if c["pm"] else None, same=same, intact=intact)
            if "noD" in c["opts"]:
                r2, same2, intact2 = _twice(lambda: call(None, None))
                res["xc_noD"] = r2[0] if c["pm"] else r2
                res["same"], res["intact"] = same and same2, intact and intact2
            self.out["conv_fwd"] = res
        return self.out["conv_fwd"]

    def comb_fwd(self):
        if "comb_fwd" not in self.out:
            from fastvim_amd import mixer_ops as M
            c, v = self.c, self.dev
            rows, cols, tr = self._geo()
            skip = self.conv_fwd()["skip"]
            r, same, intact = _twice(lambda: M.combine_fwd(v["xz"], skip, v["yc"], v["ln_w"], v["ln_b"], v["eps"], rows, cols,
                                                           tr, tpp=c["tpp"]))
            self.out["comb_fwd"] = dict(g=r[0], mean=r[1], rstd=r[2], same=same, intact=intact)
        return self.out["comb_fwd"]

    def comb_bwd(self):
        if "comb_bwd" not in self.out:
            from fastvim_amd import mixer_ops as M
            c, v = self.c, self.dev
            rows, cols, tr = self._geo()
            skip, f = self.conv_fwd()["skip"], self.comb_fwd()
            dxz = [torch.full_like(v["xz"], SENTINEL) for _ in range(2)]
            it = iter(dxz)
            r, same, intact = _twice(lambda: M.combine_bwd(v["dg"], v["xz"], skip, v["yc"], v["ln_w"], v["ln_b"], f["mean"],
                                                           f["rstd"], next(it), rows, cols, tr, tpp=c["tpp"]))
            same = same and torch.equal(dxz[0].view(torch.int16 if dxz[0].dtype == torch.bfloat16 else torch.int32),
                                        dxz[1].view(torch.int16 if dxz[1].dtype == torch.bfloat16 else torch.int32))
            self.out["comb_bwd"] = dict(d_o=r[0], dyc=r[1], dln=r[2], dxz=dxz[0], same=same, intact=intact)
        return self.out["comb_bwd"]

    def conv_bwd(self):
        if "conv_bwd" not in self.out:
            from fastvim_amd import mixer_ops as M
            c, v = self.c, self.dev
            rows, cols, tr = self._geo()
            amax = self.conv_fwd()["amax"]
            if COMB_BWD in c["plans"]:
                b = self.comb_bwd()                       # the z half of dxz holds dz, the x half the sentinel
            else:                                         # no combine adjoint at this shape: a random d_o
                b = dict(d_o=v["dg"], dxz=torch.full_like(v["xz"], SENTINEL))
            dxz = [b["dxz"].clone() for _ in range(2)]
            it = iter(dxz)
            r, same, intact = _twice(lambda: M.conv_pool_bwd(v["xz"], b["d_o"], v["dxc"], v["cw"], v["cb"], v["cwb"], v["cbb"],
                                                             v["D"], v["Db"], next(it), rows, cols, tr, c["pm"], v["scaling"],
                                                             tpp=c["tpp"], amax=amax, dxc2=v["dxc2"]))
            same = same and torch.equal(dxz[0].view(torch.int16 if dxz[0].dtype == torch.bfloat16 else torch.int32),
                                        dxz[1].view(torch.int16 if dxz[1].dtype == torch.bfloat16 else torch.int32))
            self.out["conv_bwd"] = dict(part=r, dxz=dxz[0], same=same, intact=intact, d_o=b["d_o"], dxz_in=b["dxz"])
        return self.out["conv_bwd"]


_CHAINS = {}


def chain(name):
    if name not in _CHAINS:
        if len(_CHAINS) >= 2:          # the tests of a case run back to back: keep the device memory of few
            _CHAINS.pop(next(iter(_CHAINS)))
        _CHAINS[name] = Chain(CASE_BY_NAME[name])
    return _CHAINS[name]


@pytest.fixture(scope="module")
def lib():
    import fastvim_amd.build as fb
    fb.build()
    from fastvim_amd import _lib
    return _lib.lib()


_cpu, _close = R.cpu64, R.close      # the bound helper lives in mixer_family_ref.py (test_fused_proj_gpu.py uses it too)


def _names(family):
    return [c["name"] for c in CASES if family in c["plans"]]


def _fwd_blocks(nrows, rg, cap=512):
    """Grid of the persistent forward combine kernels (persistent_blocks_f of csrc/mixer_fwd.hip, the wave kernels'
    combine_wave_blocks): the row groups dealt out evenly over at most 512 blocks."""
    groups = -(-nrows // rg)
    per = -(-groups // cap)
    return -(-groups // per)


def _assert_persistent_and_ragged(nrows, blocks, rg):
    assert blocks * rg < nrows, "one iteration covers every row: not persistent"
    nit = -(-nrows // (blocks * rg))
    assert nit * blocks * rg > nrows, "the last iteration is not ragged"


@pytest.mark.parametrize("name", _names(CONV_FWD))
def test_conv_pool_fwd_vs_fp64(lib, name):
    c = CASE_BY_NAME[name]
    assert_plan(lib, c, CONV_FWD)
    ch = chain(name)
    inp, out = ch.inp, ch.conv_fwd()
    bf = c["dt"] == "bf16"
    x = inp["xz"][..., :c["d"]]
    conv_f, conv_b, xc, skip, arg = R.conv_pool_ref(x, inp["cw"], inp["cb"], inp["cwb"], inp["cbb"], inp["D"], inp["Db"],
                                                    c["rows"], c["cols"], c["tpp"], c["pm"], inp["scaling"], c["tr"])
    errs = []
    assert out["same"], "two launches differ"
    assert out["intact"], "the kernel wrote past its outputs"
    _close(errs, "xc", out["xc"], xc, 1e-5, bf)
    _close(errs, "skip", out["skip"], skip, 1e-5, bf)
    if "noD" in c["opts"]:
        assert torch.equal(_cpu(out["xc_noD"]), _cpu(out["xc"]))
    if c["pm"]:
        got = _cpu(out["amax"])
        tie = torch.stack([near_tie_groups(conv_f, c), near_tie_groups(conv_b, c)])
        assert tie.float().mean().item() <= 0.005, tie.float().mean().item()
        assert bool((got == got.round()).all()) and bool(((got >= 0) & (got < c["cols"])).all())
        wrong = (got != arg) & ~tie
        assert not bool(wrong.any()), (int(wrong.sum()), tuple(int(k) for k in torch.unravel_index(wrong.int().argmax(), wrong.shape)))
        if "argmax_exact" in c["opts"]:      # bf16 holds every integer up to 256: columns 0..254 must come back exactly
            assert bool((got == arg)[~tie].all()) and got.max().item() > 128
    assert not errs, errs


@pytest.mark.parametrize("name", _names(COMB_FWD))
def test_combine_fwd_vs_fp64(lib, name):
    c = CASE_BY_NAME[name]
    pl = assert_plan(lib, c, COMB_FWD)
    if "persistent" in c["opts"]:
        _assert_persistent_and_ragged(c["B"] * c["rows"], _fwd_blocks(c["B"] * c["rows"], pl[4]), pl[4])
    ch = chain(name)
    inp, out = ch.inp, ch.comb_fwd()
    bf = c["dt"] == "bf16"
    z = inp["xz"][..., c["d"]:]
    o, g, mean, rstd = R.combine_ref(z, _cpu(ch.conv_fwd()["skip"]), inp["yc"], inp["ln_w"], inp["ln_b"], inp["eps"],
                                     c["rows"], c["cols"], c["tpp"], c["tr"])
    if "offset" in c["opts"]:
        assert (o.mean(-1).abs() / o.std(-1)).min().item() >= 30.0
    errs = []
    assert out["same"], "two launches differ"
    assert out["intact"], "the kernel wrote past its outputs"
    _close(errs, "g", out["g"], g, 1e-5, bf)
    if inp["ln_w"] is not None:
        _close(errs, "mean", out["mean"], mean, 1e-5, elementwise_scale=True)
        _close(errs, "rstd", out["rstd"], rstd, 1e-5, elementwise_scale=True)
    assert not errs, errs


@pytest.mark.parametrize("name", _names(COMB_BWD))
def test_combine_bwd_vs_fp64(lib, name):
    c = CASE_BY_NAME[name]
    pl = assert_plan(lib, c, COMB_BWD)
    if "persistent" in c["opts"]:
        i = ctypes.c_int
        _assert_persistent_and_ragged(c["B"] * c["rows"], lib.fv_mixer_bwd_blocks(i(c["B"]), i(c["rows"]), i(c["d"]), i(c["tpp"]), i(0)), pl[4])
    ch = chain(name)
    inp, out = ch.inp, ch.comb_bwd()
    bf = c["dt"] == "bf16"
    d = c["d"]
    z = inp["xz"][..., d:]
    dz, d_o, dyc, dlw, dlb = R.combine_adjoint_ref(inp["dg"], z, _cpu(ch.conv_fwd()["skip"]), inp["yc"], inp["ln_w"],
                                                   inp["ln_b"], inp["eps"], c["rows"], c["cols"], c["tpp"], c["tr"])
    errs = []
    assert out["same"], "two launches differ"
    assert out["intact"], "the kernel wrote past its outputs"
    _close(errs, "dz", out["dxz"][..., d:], dz, 2e-5, bf)
    assert bool((out["dxz"][..., :d] == SENTINEL).all()), "combine_bwd touched the x half of dxz"
    _close(errs, "d_o", out["d_o"], d_o, 2e-5, bf)
    _close(errs, "dyc", out["dyc"], dyc, 5e-5)
    if inp["ln_w"] is not None:
        _close(errs, "d ln_w", out["dln"][0], dlw, 1e-4)
        _close(errs, "d ln_b", out["dln"][1], dlb, 1e-4)
    assert not errs, errs


@pytest.mark.parametrize("name", _names(CONV_BWD))
def test_conv_pool_bwd_vs_fp64(lib, name):
    c = CASE_BY_NAME[name]
    pl = assert_plan(lib, c, CONV_BWD)
    assert bool(pl[6]) or "dxc2" not in c["opts"]
    if "persistent" in c["opts"]:
        i = ctypes.c_int
        _assert_persistent_and_ragged(c["B"] * c["rows"], lib.fv_mixer_bwd_blocks(i(c["B"]), i(c["rows"]), i(c["d"]), i(c["tpp"]), i(1)), pl[4])
    ch = chain(name)
    inp, out = ch.inp, ch.conv_bwd()
    bf = c["dt"] == "bf16"
    d = c["d"]
    x = inp["xz"][..., :d]
    dx, part = R.conv_pool_adjoint_ref(x, inp["cw"], inp["cb"], inp["cwb"], inp["cbb"], inp["D"], inp["Db"],
                                       _cpu(out["d_o"]), inp["dxc"], c["rows"], c["cols"], c["tpp"], c["pm"],
                                       inp["scaling"], c["tr"], amax=_cpu(ch.conv_fwd()["amax"]), dxc2=inp["dxc2"])
    errs = []
    assert out["same"], "two launches differ"
    assert out["intact"], "the kernel wrote past its outputs"
    _close(errs, "dx", out["dxz"][..., :d], dx, 2e-5, bf)
    assert torch.equal(_cpu(out["dxz"][..., d:]), _cpu(out["dxz_in"][..., d:])), "conv_pool_bwd touched the z half of dxz"
    got = _cpu(out["part"]).reshape(-1)
    seg = dict(dw=(0, 4 * d), dw_b=(4 * d, 8 * d), db=(8 * d, 9 * d), db_b=(9 * d, 10 * d), dD=(10 * d, 11 * d), dD_b=(11 * d, 12 * d))
    for k, (lo, hi) in seg.items():
        if k in ("db", "db_b") and inp["cb"] is None:
            continue
        _close(errs, k, got[lo:hi], part[lo:hi], 1e-4)
    assert not errs, errs


def test_conv_pool_bwd_refuses_rows_shorter_than_the_halo(lib):
    """The adjoint kernels keep the pooled gradients of rows i-1, i, i+1 only: fewer than 3 tokens per pooling row is an
    error there (the forward serves such rows: the `short` cases above)."""
    from fastvim_amd import mixer_ops as M
    for cols in (1, 2):
        ch = Chain(_case("refuse", 64, 4, cols, "CF:G1", seed=7))
        v = ch.dev
        dxz = torch.zeros_like(v["xz"])
        with pytest.raises(RuntimeError, match="at least 3 tokens"):
            M.conv_pool_bwd(v["xz"], v["dg"], v["dxc"], v["cw"], v["cb"], v["cwb"], v["cbb"], v["D"], v["Db"], dxz, 4, cols,
                            False, 0, 1.0)
        assert not bool(dxz.any())
