"""Launch plans of the un-pooled geometry (one patch column, tokens_per_patch = t: every token its own pooling group),
the form the masked MAE encoders and the un-pooled Vim mixer launch, at the FastVim-L / -H widths (csrc/mixer_plan.h
through fv_mixer_plan).  Host code only."""
import ctypes

import pytest

CONV_FWD, COMB_FWD, COMB_BWD, CONV_BWD = 0, 1, 2, 3
UNSUPPORTED, GENERIC, ROW, CELL, WAVE = 0, 1, 2, 3, 4
F32, BF16 = 0, 1
UNPOOLED = [(1, 10), (7, 7), (16, 4), (8, 8), (5, 3)]      # (rows, tokens_per_patch)


@pytest.fixture(scope="module")
def lib():
    import fastvim_amd.build as fb
    fb.build()
    from fastvim_amd import _lib
    return _lib.lib()


def _plan(lib, family, d, cols=1, rows=7, tpp=7, pool_max=0, dtype=BF16, batch=2):
    out = (ctypes.c_int * 8)()
    i = ctypes.c_int
    rc = lib.fv_mixer_plan(i(family), i(batch), i(rows), i(cols), i(tpp), i(d), i(pool_max), i(dtype), out)
    assert rc == 0
    return tuple(out)[:7]      # form, vec, waves, slabs, row_groups, lds_bytes, takes_dxc2


@pytest.mark.parametrize("d", [2048, 2560])
def test_l_and_h_widths_are_supported_in_all_four_families_unpooled(lib, d):
    for fam in (CONV_FWD, COMB_FWD, COMB_BWD, CONV_BWD):
        for rows, tpp in UNPOOLED:
            for dt in (F32, BF16):
                assert _plan(lib, fam, d, rows=rows, tpp=tpp, dtype=dt)[0] != UNSUPPORTED, (fam, d, rows, tpp, dt)
    if d == 2560:      # the combine row in one block: 5 waves x 8 channels per lane
        assert _plan(lib, COMB_FWD, d)[:5] == (GENERIC, 8, 5, 1, 1) and _plan(lib, COMB_BWD, d)[:5] == (GENERIC, 8, 5, 1, 1)


def test_every_supported_unpooled_plan_fits_the_hardware_and_covers_d_inner(lib):
    for d in range(64, 3072 + 1, 64):
        for fam in (CONV_FWD, COMB_FWD, COMB_BWD, CONV_BWD):
            for rows, tpp in UNPOOLED:
                for dt in (F32, BF16):
                    form, vec, waves, slabs, rg, lds, dxc2 = _plan(lib, fam, d, rows=rows, tpp=tpp, dtype=dt)
                    if form == UNSUPPORTED:
                        continue
                    assert form in (GENERIC, ROW, CELL, WAVE)
                    assert 1 <= waves * rg * 64 <= 1024, (fam, d, rows, tpp)
                    assert 0 <= lds <= 160 * 1024, (fam, d, rows, tpp)
                    assert slabs * waves * 64 * vec == d, (fam, d, rows, tpp, (vec, waves, slabs))
                    if fam in (COMB_FWD, COMB_BWD):
                        assert slabs == 1          # LayerNorm statistics run over the whole row
                    assert not dxc2


def test_wide_combine_is_the_only_fit_for_the_multiples_of_512(lib):
    """Multiples of 512 above 1024 up to 4096 that no narrower form holds take 8 channels per lane."""
    for d in (2560, 3584, 4096):
        for fam in (COMB_FWD, COMB_BWD):
            assert _plan(lib, fam, d)[:5] == (GENERIC, 8, d // 512, 1, 1), (fam, d)
    assert _plan(lib, COMB_BWD, 3072)[:5] == (GENERIC, 8, 6, 1, 1)       # forward: 6 channels per lane on 8 waves
    assert _plan(lib, COMB_FWD, 3072)[:5] == (GENERIC, 6, 8, 1, 1)


def test_channel_model_geometry_stays_unsupported_at_2560(lib):
    """tokens_per_patch 8 with 14 patch columns needs the LDS slot accumulators: no reference model has it at 2560."""
    for fam in (COMB_FWD, COMB_BWD):
        for dt in (F32, BF16):
            assert _plan(lib, fam, 2560, cols=14, rows=14, tpp=8, dtype=dt)[0] == UNSUPPORTED


# Printed from the parent commit's library (before the plan rule changed): what the un-pooled models launch at the
# widths they were served at does not move.  (family, tokens_per_patch = rows) -> {d_inner: plan}; fp32 and bf16
# storage gave the same rows.
PARENT = {
    (CONV_FWD, 7): {384: (1, 2, 3, 1, 1, 0, 0), 768: (1, 2, 6, 1, 1, 0, 0), 1024: (1, 2, 8, 1, 1, 0, 0), 1536: (1, 4, 6, 1, 1, 0, 0)},
    (CONV_FWD, 8): {384: (1, 2, 3, 1, 1, 0, 0), 768: (1, 2, 6, 1, 1, 0, 0), 1024: (1, 2, 8, 1, 1, 0, 0), 1536: (1, 4, 6, 1, 1, 0, 0)},
    (COMB_FWD, 7): {384: (4, 6, 1, 1, 4, 0, 0), 768: (4, 12, 1, 1, 4, 0, 0), 1024: (1, 4, 4, 1, 2, 256, 0), 1536: (4, 24, 1, 1, 4, 0, 0)},
    (COMB_FWD, 8): {384: (4, 6, 1, 1, 4, 0, 0), 768: (4, 12, 1, 1, 4, 0, 0), 1024: (1, 4, 4, 1, 2, 512, 0), 1536: (4, 24, 1, 1, 4, 0, 0)},
    (COMB_BWD, 7): {384: (4, 6, 1, 1, 4, 3072, 0), 768: (4, 12, 1, 1, 4, 6144, 0), 1024: (1, 2, 8, 1, 1, 8704, 0), 1536: (4, 24, 1, 1, 4, 12288, 0)},
    (COMB_BWD, 8): {384: (4, 6, 1, 1, 4, 3072, 0), 768: (4, 12, 1, 1, 4, 6144, 0), 1024: (1, 2, 8, 1, 1, 9216, 0), 1536: (4, 24, 1, 1, 4, 12288, 0)},
    (CONV_BWD, 7): {384: (1, 2, 3, 1, 4, 18432, 0), 768: (1, 2, 6, 1, 2, 36864, 0), 1024: (1, 2, 8, 1, 1, 49152, 0), 1536: (1, 2, 12, 1, 1, 73728, 0)},
    (CONV_BWD, 8): {384: (1, 2, 3, 1, 4, 18432, 0), 768: (1, 2, 6, 1, 2, 36864, 0), 1024: (1, 2, 8, 1, 1, 49152, 0), 1536: (1, 2, 12, 1, 1, 73728, 0)},
}


@pytest.mark.parametrize("key", sorted(PARENT))
def test_unpooled_plans_of_the_served_widths_are_the_parents(lib, key):
    fam, t = key
    for d, want in PARENT[key].items():
        for dt in (F32, BF16):
            assert _plan(lib, fam, d, rows=t, tpp=t, dtype=dt) == want, (fam, t, d, dt)


def test_partial_rows_follow_the_unpooled_plan(lib):
    """fv_mixer_bwd_blocks has no column argument: the combine adjoint's partial rows must follow the one-column plan."""
    i = ctypes.c_int
    for d in (1024, 2048, 2560, 3072):
        for rows, tpp in UNPOOLED:
            vec, rg = _plan(lib, COMB_BWD, d, rows=rows, tpp=tpp)[1], _plan(lib, COMB_BWD, d, rows=rows, tpp=tpp)[4]
            walked = 2 * rows * (tpp if vec == 8 else 1)      # 8 channels per lane: launched as rows*tpp one-token rows
            assert lib.fv_mixer_bwd_blocks(i(2), i(rows), i(d), i(tpp), i(0)) == -(-walked // rg), (d, rows, tpp)
