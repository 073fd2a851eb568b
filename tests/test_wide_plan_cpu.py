"""The launch plans of the mixer's four row-kernel families (csrc/mixer_plan.h through fv_mixer_plan): host code only,
checked without a GPU.  The launchers ask the same functions before they launch, and fv_mixer_conv_pool_bwd2_ok is
defined from the adjoint's plan, so what holds here holds for the dispatch."""
import ctypes

import pytest

CONV_FWD, COMB_FWD, COMB_BWD, CONV_BWD = 0, 1, 2, 3
UNSUPPORTED, GENERIC, ROW, CELL, WAVE = 0, 1, 2, 3, 4
F32, BF16 = 0, 1


@pytest.fixture(scope="module")
def lib():
    import fastvim_amd.build as fb
    fb.build()
    from fastvim_amd import _lib
    return _lib.lib()


def _plan(lib, family, d, cols=14, rows=14, tpp=1, pool_max=0, dtype=BF16, batch=2):
    out = (ctypes.c_int * 8)()
    i = ctypes.c_int
    rc = lib.fv_mixer_plan(i(family), i(batch), i(rows), i(cols), i(tpp), i(d), i(pool_max), i(dtype), out)
    assert rc == 0
    return tuple(out)[:7]      # form, vec, waves, slabs, row_groups, lds_bytes, takes_dxc2


SHAPES = [dict(cols=14), dict(cols=16), dict(cols=14, dtype=F32), dict(cols=5), dict(cols=7, rows=3), dict(cols=32, rows=2),
          dict(cols=14, pool_max=1), dict(cols=16, pool_max=1, dtype=F32)]


def test_every_supported_plan_fits_the_hardware_and_covers_d_inner(lib):
    for d in range(64, 3072 + 1, 64):
        for fam in (CONV_FWD, COMB_FWD, COMB_BWD, CONV_BWD):
            for kw in SHAPES:
                form, vec, waves, slabs, rg, lds, dxc2 = _plan(lib, fam, d, **kw)
                if form == UNSUPPORTED:
                    continue
                assert form in (GENERIC, ROW, CELL, WAVE)
                assert 1 <= waves * rg * 64 <= 1024, (fam, d, kw)
                assert 0 <= lds <= 160 * 1024, (fam, d, kw)
                assert slabs * waves * 64 * vec == d, (fam, d, kw, (vec, waves, slabs))
                if fam in (COMB_FWD, COMB_BWD):
                    assert slabs == 1          # LayerNorm statistics run over the whole row
                assert not dxc2 or (fam == CONV_BWD and form == ROW)


@pytest.mark.parametrize("d", [2048, 2560])
def test_fastvim_l_and_h_widths_are_supported_in_all_four_families(lib, d):
    for fam in (CONV_FWD, COMB_FWD, COMB_BWD, CONV_BWD):
        for kw in SHAPES + [dict(cols=10, rows=1), dict(cols=1, rows=1, tpp=10) if d == 2048 else dict(cols=3)]:
            assert _plan(lib, fam, d, **kw)[0] != UNSUPPORTED, (fam, d, kw)
    # the 224 px grids take the whole-row adjoint, the one form with the second pooled-gradient addend
    for cols in (14, 16):
        for dt in (F32, BF16):
            p = _plan(lib, CONV_BWD, d, cols=cols, dtype=dt)
            assert p[0] == ROW and p[1] == 2 and p[6] == 1 and p[5] <= 64 * 1024, p
    # combine: one block holds the whole row
    assert _plan(lib, COMB_FWD, 2560)[:5] == (GENERIC, 8, 5, 1, 1) and _plan(lib, COMB_BWD, 2560)[:5] == (GENERIC, 8, 5, 1, 1)
    assert _plan(lib, COMB_FWD, 2048)[:5] == (GENERIC, 4, 8, 1, 1) and _plan(lib, COMB_BWD, 2048)[:5] == (GENERIC, 4, 8, 1, 1)
    # generic conv + pool kernels (odd columns, max pooling): two channel slabs where one block cannot hold the row
    assert _plan(lib, CONV_BWD, d, cols=5)[:5] == (GENERIC, 2, d // 256, 2, 1)
    assert _plan(lib, CONV_FWD, d, cols=5)[:4] == ((GENERIC, 4, 8, 1) if d == 2048 else (GENERIC, 4, 5, 2))


def test_bwd2_predicate_follows_the_adjoint_plan(lib):
    i = ctypes.c_int
    for d in range(64, 3072 + 1, 64):
        for cols in (14, 16, 5, 32):
            for pool_max in (0, 1):
                ok = bool(lib.fv_mixer_conv_pool_bwd2_ok(i(14), i(cols), i(1), i(d), i(pool_max)))
                for dt in (F32, BF16):
                    takes = bool(_plan(lib, CONV_BWD, d, cols=cols, pool_max=pool_max, dtype=dt)[6])
                    assert ok == takes, (d, cols, pool_max, dt)
    ok = lambda d: bool(lib.fv_mixer_conv_pool_bwd2_ok(i(14), i(14), i(1), i(d), i(0)))
    assert ok(384) and ok(1536) and ok(2048) and ok(2560)
    assert not ok(1664) and not ok(1920)        # 13 / 15 waves of channel pairs: no form (the old predicate said yes)
    assert not lib.fv_mixer_conv_pool_bwd2_ok(i(14), i(14), i(2), i(384), i(0))


# The plans of the widths the kernels served before d_inner 2048 / 2560, derived by hand from the dispatch rules of the
# commit before this file (vec_combine_f / rg_combine_f, vec_combine / rg_combine, vec_convpool / rg_convpool,
# launch_row / chan_groups of the forward row kernels, the group loop of conv_pool_bwd_row):
#   (family, shape) -> {d_inner: (form, vec, waves, slabs, row_groups, lds_bytes, takes_dxc2)}
PINNED = [
    # conv + pool forward: whole-row kernel, a channel pair per lane, blocks of <= 4 waves over blockIdx.z
    (CONV_FWD, dict(cols=14), {384: (ROW, 2, 3, 1, 1, 0, 0), 768: (ROW, 2, 3, 2, 1, 0, 0),
                               1024: (ROW, 2, 4, 2, 1, 0, 0), 1536: (ROW, 2, 4, 3, 1, 0, 0)}),
    # odd columns / max pooling: the tile kernel, 6 or 4 channels per lane
    (CONV_FWD, dict(cols=5), {384: (GENERIC, 6, 1, 1, 1, 0, 0), 768: (GENERIC, 6, 2, 1, 1, 0, 0),
                              1024: (GENERIC, 4, 4, 1, 1, 0, 0), 1536: (GENERIC, 6, 4, 1, 1, 0, 0)}),
    (CONV_FWD, dict(cols=14, pool_max=1), {384: (GENERIC, 6, 1, 1, 1, 0, 0), 1024: (GENERIC, 4, 4, 1, 1, 0, 0)}),
    # long dense rows: cell walker, blocks of <= 2 waves
    (CONV_FWD, dict(cols=32), {384: (CELL, 2, 1, 3, 1, 0, 0), 768: (CELL, 2, 2, 3, 1, 0, 0),
                               1024: (CELL, 2, 2, 4, 1, 0, 0), 1536: (CELL, 2, 2, 6, 1, 0, 0)}),
    # combine forward: wave per token at 384 / 768 / 1536, else 4 channels per lane and two row groups
    (COMB_FWD, dict(cols=14), {384: (WAVE, 6, 1, 1, 4, 0, 0), 768: (WAVE, 12, 1, 1, 4, 0, 0),
                               1024: (GENERIC, 4, 4, 1, 2, 512, 0), 1536: (WAVE, 24, 1, 1, 4, 0, 0)}),
    (COMB_FWD, dict(cols=5), {1024: (GENERIC, 4, 4, 1, 2, 256, 0)}),
    (COMB_BWD, dict(cols=14), {384: (WAVE, 6, 1, 1, 4, 3072, 0), 768: (WAVE, 12, 1, 1, 4, 6144, 0),
                               1024: (GENERIC, 4, 4, 1, 2, 9216, 0), 1536: (WAVE, 24, 1, 1, 4, 12288, 0)}),
    (COMB_BWD, dict(cols=5), {1024: (GENERIC, 4, 4, 1, 2, 8704, 0)}),
    # conv + pool adjoint, whole-row kernel: bf16 14-column rows fill 12 waves, everything else 8
    (CONV_BWD, dict(cols=14, dtype=BF16), {384: (ROW, 2, 3, 1, 4, 18432, 1), 768: (ROW, 2, 6, 1, 2, 36864, 1),
                                           1024: (ROW, 2, 4, 2, 1, 49152, 1), 1536: (ROW, 2, 12, 1, 1, 73728, 1)}),
    (CONV_BWD, dict(cols=14, dtype=F32), {384: (ROW, 2, 1, 3, 4, 18432, 1), 768: (ROW, 2, 2, 3, 2, 36864, 1),
                                          1024: (ROW, 2, 8, 1, 1, 49152, 1), 1536: (ROW, 2, 4, 3, 1, 73728, 1)}),
    (CONV_BWD, dict(cols=16, dtype=BF16), {384: (ROW, 2, 1, 3, 4, 18432, 1), 1536: (ROW, 2, 4, 3, 1, 73728, 1)}),
    # streaming kernel: a channel pair per lane, row groups while 12 waves allow
    (CONV_BWD, dict(cols=5), {384: (GENERIC, 2, 3, 1, 4, 18432, 0), 768: (GENERIC, 2, 6, 1, 2, 36864, 0),
                              1024: (GENERIC, 2, 8, 1, 1, 49152, 0), 1536: (GENERIC, 2, 12, 1, 1, 73728, 0)}),
    (CONV_BWD, dict(cols=14, pool_max=1), {768: (GENERIC, 2, 6, 1, 2, 36864, 0)}),
    # long dense rows: cell walker, four-wave blocks that accumulate their own channels
    (CONV_BWD, dict(cols=32), {384: (CELL, 2, 1, 3, 4, 6144, 0), 768: (CELL, 2, 2, 3, 2, 12288, 0),
                               1024: (CELL, 2, 2, 4, 2, 12288, 0), 1536: (CELL, 2, 2, 6, 2, 12288, 0)}),
]


@pytest.mark.parametrize("k", range(len(PINNED)))
def test_plans_of_the_served_widths_are_the_parent_dispatch(lib, k):
    fam, kw, table = PINNED[k]
    for d, want in table.items():
        assert _plan(lib, fam, d, **kw) == want, (fam, kw, d)


def test_partial_rows_follow_the_plan(lib):
    """fv_mixer_bwd_blocks (rows of gradient partials Python allocates) uses the plan's row groups."""
    i = ctypes.c_int
    for d, rows_per_block in ((384, 4), (768, 2), (1024, 1), (1536, 1), (2048, 1), (2560, 1)):
        nb = lib.fv_mixer_bwd_blocks(i(2), i(14), i(d), i(1), i(1))
        assert nb == -(-28 // rows_per_block), (d, nb)
    assert lib.fv_mixer_bwd_blocks(i(2), i(14), i(2560), i(1), i(0)) == 28       # combine: one row group per block
    assert lib.fv_mixer_bwd_blocks(i(2), i(14), i(1024), i(1), i(0)) == 14
