"""Device-side cell augmentation (fastvim_amd/cellaug.py, csrc/cellaug.hip) against its numpy restatement
(tests/cellaug_ref.py, itself held to scipy by tests/test_cellaug_cpu.py).  Every comparison is ``torch.equal``.

Shapes are the smallest at which the kernels can go wrong.  B = 6 with FORCED plans, so that every geometry op, both defocus
states and both hole states occur in one batch (two such batches: rotations by 0, 90, -133.7 and 270 degrees, radius 1 and
3, 0 and 10 holes, one of them on the border).  C in {1, 3, 8}.  S = 16 (one partial tile) and 40 (two tiles per axis: halos
cross a tile edge and reflect at both borders); S = 70 as well (three 32-column tiles, and 70 % 4 != 0: the
byte-store path).  Sources smaller than S (9 x 13, padded), larger (50 x 37) and with odd H * W (plane bases at odd
addresses)."""
import functools

import numpy as np
import pytest
import torch

import cellaug_ref as R

pytestmark = pytest.mark.gpu

SIZES = ((9, 13), (50, 37), (45, 37), (16, 40), (71, 5), (33, 33))
CASES = [(c, s) for s in (16, 40) for c in (1, 3, 8)] + [(3, 70)]


def _holes(S, seed, border):
    rng = np.random.default_rng(seed)
    holes = []
    for k in range(10):
        h, w = int(rng.integers(1, 7)), int(rng.integers(1, 7))
        y, x = int(rng.integers(0, S - h + 1)), int(rng.integers(0, S - w + 1))
        holes.append((y, x, y + h, x + w))
    if border:
        holes[0] = (S - 3, S - 5, S, S)
        holes[1] = (0, 0, 2, S)
    return holes


def _plans(S, which):
    from fastvim_amd.cellaug import CellPlan, HFLIP, NONE, ROTATE, VFLIP
    if which == 0:
        return [CellPlan(3, 2, NONE),                                                        # 9 x 13: padded on every side
                CellPlan(-20, -11, HFLIP, radius=1, sigma=0.1, holes=_holes(S, 1, True)),     # 50 x 37 from (20, 11)
                CellPlan(-2, 1, VFLIP, radius=3, sigma=0.5),
                CellPlan(0, 0, ROTATE, 90.0, holes=_holes(S, 2, False)),
                CellPlan(-30, 4, ROTATE, -133.7, radius=3, sigma=0.33, holes=_holes(S, 3, True)),
                CellPlan(S - 4, S - 4, ROTATE, 270.0, radius=1, sigma=0.5)]                  # a 4 x 4 corner of the source
    return [CellPlan(1, -4, ROTATE, 0.0),                                                    # the identity through the taps
            CellPlan(0, 0, ROTATE, 17.3, radius=2, sigma=0.2),
            CellPlan(-41, -30, HFLIP, holes=_holes(S, 4, True)),                             # the source ends inside the crop
            CellPlan(5, 5, VFLIP, radius=2, sigma=0.45, holes=_holes(S, 5, False)),
            CellPlan(S, 0, NONE, radius=3, sigma=0.1),                                       # nothing of the source: zeros
            CellPlan(-3, -3, NONE, holes=[(0, 0, S, S)])]                                    # one hole over everything


@functools.lru_cache(maxsize=None)
def _batch(C, S, which):
    """Sources, plans and the restatement's two stages for one forced batch (computed once, never modified)."""
    rng = np.random.default_rng(100 * C + S + which)
    srcs = [rng.integers(0, 256, (C,) + hw, dtype=np.uint8) for hw in SIZES]
    plans = _plans(S, which)
    g = np.stack([R.geom(a, S, p.oy, p.ox, p.op, R.rotation_matrix(S, S, p.angle)) for a, p in zip(srcs, plans)])
    noise = rng.integers(0, 256, g.shape, dtype=np.uint8)
    f = np.stack([R.filter(n, R.defocus_kernel(p.radius, p.sigma) if p.radius else None, p.holes) for n, p in zip(noise, plans)])
    full = np.stack([R.apply(a, S, p) for a, p in zip(srcs, plans)])
    for t in (g, noise, f, full):
        t.setflags(write=False)
    return srcs, plans, g, noise, f, full


def _staged(C, S, srcs, plans):
    """Pool and plan table on the device, through the host half alone."""
    from fastvim_amd.cellaug import HostCellPlan
    host = HostCellPlan(len(srcs), C, S, 1 << 17)
    for k, (a, p) in enumerate(zip(srcs, plans)):
        host.put(k, a, p)
    return torch.from_numpy(host.pool).cuda(), torch.from_numpy(host.plan).cuda()


def _mismatch(got, want):
    return [(b, int((got[b] != want[b]).sum())) for b in range(got.shape[0]) if not torch.equal(got[b], want[b])]


def _eq(got, want):
    got, want = got.cpu(), torch.from_numpy(np.array(want))               # (a copy: the cached references are read-only)
    assert torch.equal(got, want), _mismatch(got, want)


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("C,S", CASES)
def test_geom_alone(C, S, which):
    from fastvim_amd import cellaug as CA
    srcs, plans, g, _, _, _ = _batch(C, S, which)
    pool, plan = _staged(C, S, srcs, plans)
    out = torch.full((6, C, S, S), 77, dtype=torch.uint8, device="cuda")
    CA.geom(pool, plan, out)
    _eq(out, g)
    if which == 1:
        crop = R.geom(srcs[0], S, 1, -4)
        assert np.array_equal(out[0].cpu().numpy(), crop) and (out[4] == 0).all()          # rotation by 0; nothing in view


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("C,S", CASES)
def test_filter_alone(C, S, which):
    from fastvim_amd import cellaug as CA
    srcs, plans, _, noise, f, _ = _batch(C, S, which)
    _, plan = _staged(C, S, srcs, plans)
    out = torch.full((6, C, S, S), 77, dtype=torch.uint8, device="cuda")
    CA.filter(torch.from_numpy(noise.copy()).cuda(), plan, out)
    _eq(out, f)
    if which == 0:
        assert np.array_equal(out[0].cpu().numpy(), noise[0])                              # no defocus, no holes: a copy
    with pytest.raises(RuntimeError, match="overlap"):
        CA.filter(out, plan, out)


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("C,S", CASES)
def test_pair_through_the_stage(C, S, which):
    from fastvim_amd.cellaug import CellStage
    srcs, plans, _, _, _, full = _batch(C, S, which)
    stage = CellStage(6, channels=C, out_size=S, capacity_bytes=1 << 17, slots=1)
    for k in (3, 0, 5, 1, 4, 2):                                                           # any order
        stage.put(k, srcs[k], plans[k])
    stage.commit()
    out = torch.full((6, C, S, S), 77, dtype=torch.uint8, device="cuda")
    assert stage.apply(out=out) is out
    _eq(out, full)


def test_unaligned_out_takes_the_byte_path():
    """S % 4 == 0 but the planes start at an odd address: no 4-byte access anywhere."""
    from fastvim_amd import cellaug as CA
    C, S = 3, 16
    srcs, plans, g, noise, f, _ = _batch(C, S, 0)
    pool, plan = _staged(C, S, srcs, plans)
    n = 6 * C * S * S
    buf = torch.full((n + 1,), 77, dtype=torch.uint8, device="cuda")
    out = buf[1:].view(6, C, S, S)
    CA.geom(pool, plan, out)
    _eq(out, g)
    inp = torch.empty(n + 1, dtype=torch.uint8, device="cuda")[1:].view(6, C, S, S)
    inp.copy_(torch.from_numpy(noise.copy()))
    CA.filter(inp, plan, out)
    _eq(out, f)
    assert buf[0].item() == 77


def _drawn(aug, rng, B, C, S):
    srcs = [rng.integers(0, 256, (C, int(rng.integers(S // 2, 3 * S)), int(rng.integers(S // 2, 3 * S))), dtype=np.uint8)
            for _ in range(B)]
    return srcs, [aug.draw(a.shape[1], a.shape[2]) for a in srcs]


def test_drawn_batches_through_two_slots():
    from fastvim_amd.cellaug import CellAugmentation, CellStage
    B, C, S = 8, 3, 40
    aug = CellAugmentation(S, seed=5, min_side=48, max_height=6, max_width=6)
    rng = np.random.default_rng(6)
    stage = CellStage(B, channels=C, out_size=S, capacity_bytes=B * C * 120 * 120, slots=2)
    outs = [torch.full((B, C, S, S), 77, dtype=torch.uint8, device="cuda") for _ in range(3)]
    wants = []
    for out in outs:                                   # nothing waits between the rounds: slot 0 is reused by the third
        srcs, plans = _drawn(aug, rng, B, C, S)
        for k in range(B):
            stage.put(k, srcs[k], plans[k])
        stage.commit()
        stage.apply(out=out)
        wants.append(np.stack([R.apply(a, S, p) for a, p in zip(srcs, plans)]))
    for out, want in zip(outs, wants):
        _eq(out, want)
    assert stage.staged_bytes > 0
    # validation: no plan is the identity
    val = [rng.integers(0, 256, (C, S, S), dtype=np.uint8) for _ in range(B)]
    for k in range(B):
        stage.put(k, val[k], None)
    stage.commit()
    stage.apply(out=outs[0])
    _eq(outs[0], np.stack(val))
    with pytest.raises(ValueError, match="without a plan"):
        stage.put(0, np.zeros((C, S, S + 1), np.uint8), None)


def test_graph_replay_reads_the_plan_and_the_pool_of_the_moment():
    from fastvim_amd.cellaug import CellAugmentation, CellStage
    B, C, S = 6, 3, 40
    aug = CellAugmentation(S, seed=9, min_side=48, p_flip_rotate=0.9, p_defocus=0.7, max_height=6, max_width=6)
    rng = np.random.default_rng(10)
    stage = CellStage(B, channels=C, out_size=S, capacity_bytes=B * C * 120 * 120, slots=1)
    x = torch.zeros(B, C, S, S, dtype=torch.uint8, device="cuda")

    def fill():
        srcs, plans = _drawn(aug, rng, B, C, S)
        for k in range(B):
            stage.put(k, srcs[k], plans[k])
        stage.commit()
        return np.stack([R.apply(a, S, p) for a, p in zip(srcs, plans)])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        want = fill()
        stage.apply(out=x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _eq(x, want)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stage.apply(out=x)
    for _ in range(2):
        want = fill()                                  # a new plan and new pool contents, written between replays
        graph.replay()
        _eq(x, want)
        eager = torch.full_like(x, 77)
        stage.apply(out=eager)
        assert torch.equal(eager, x)


def test_unfold_of_the_stage_output():
    """End to end into the channel models' first launch: ``fv_patch_unfold_chan_u8`` on the stage's bytes."""
    from fastvim_amd import glue_ops as G
    from fastvim_amd.cellaug import CellStage
    from fastvim_amd.pixels import PixelNorm
    C, S = 8, 16
    srcs, plans, _, _, _, full = _batch(C, S, 0)
    stage = CellStage(6, channels=C, out_size=S, capacity_bytes=1 << 17, slots=1)
    for k in range(6):
        stage.put(k, srcs[k], plans[k])
    stage.commit()
    x = torch.empty(6, C, S, S, dtype=torch.uint8, device="cuda")
    stage.apply(out=x)
    pn = PixelNorm(tuple(0.05 + 0.04 * c for c in range(C)), tuple(0.02 + 0.03 * c for c in range(C)), formula="albumentations")
    table = pn.table(x.device)
    assert G.patch_unfold_chan_u8_ok(x, 8, 8, C)
    sel = torch.tensor([5, 0, 7, 2], dtype=torch.int32, device="cuda")
    want_x = torch.from_numpy(full.copy()).cuda()
    for s, n in ((None, C), (sel, 4)):
        got = G.patch_unfold_chan_u8(x, table, 8, 8, torch.bfloat16, s, n)
        assert torch.equal(got, G.patch_unfold_chan_u8(want_x, table, 8, 8, torch.bfloat16, s, n))
    assert torch.equal(x, want_x)
