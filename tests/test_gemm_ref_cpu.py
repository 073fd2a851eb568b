"""tests/gemm_ref.py on the CPU: the fp32 emulation stays inside every per-element bound on every case of
tests/test_gemm_plans_gpu.py, the bounds catch two injected faults in every tile, every plan key a sweep over the rule
boundaries reaches at 256 CUs has a case, and the keys left out stay unreachable.  The plan queries are host code of the
library: no GPU is needed."""
import pytest
import torch

import gemm_ref as R

CUS = 256
CPU_FULL = 3e8        # multiply-adds up to which this file checks every row of a case; above, the rows of R.sample_rows


@pytest.fixture(scope="module")
def lib():
    import fastvim_amd.build as fb
    fb.build()
    return R.host_lib()


def _checked(c, seed):
    """One case on the CPU, computed once: per K slice (rows, target, bound, emulation, emulation with the last k dropped)."""
    A, B, bias = R.operands(c, seed)
    rows = torch.arange(c["M"]) if R.macs(c) <= CPU_FULL else R.sample_rows(c["M"], c["tile"][0], seed)
    A = A[rows]
    A64, B64 = A.double(), B.double()
    b64 = None if bias is None else bias.double()
    out = []
    for k0, k1 in R.slices(c["K"], c["splits"]):
        P, S = R.reference(A64, B64, k0, k1)
        target, bnd = R.bound(P, S, k1 - k0, c["c_fp32"], b64)
        out.append((rows, target, bnd, R.emulate(A, B, k0, k1, c["c_fp32"], bias),
                    R.emulate(A, B, k0, k1, c["c_fp32"], bias, drop_last=True) if c["c_fp32"] else None))
    return out


@pytest.fixture(scope="module")
def checked(lib):
    res = []
    for i, c in enumerate(R.gemm_cases(CUS)):
        p = R.plan(c["M"], c["N"], c["K"], c["a_ks"], c["b_ks"], c["c_fp32"], c["bias"], c["N"] + c["ldc_pad"], c["splits"], CUS)
        c["tile"] = (p[1], p[2])
        res.append((c, _checked(c, 1000 + i)))
    for i, g in enumerate(R.grouped_cases()):
        launches = R.grouped_launches(g["problems"])
        for l, key in zip(launches, g["keys"]):
            for j, q in enumerate(l[:3]):         # (a launch's problems beyond the third repeat their shapes)
                c = dict(name=f"{g['name']}_{j}", M=q["M"], N=q["N"], K=q["Kd"], c_fp32=1, bias=0, splits=max(q["splits"], 1),
                         tile=R.GROUPED_TILES[key[0]])
                res.append((c, _checked(c, 2000 + 50 * i + j)))
    return res


def test_emulation_is_inside_every_bound(checked):
    worst = {"bf16": 0.0, "fp32": 0.0}
    for c, sl in checked:
        for rows, target, bnd, emu, _ in sl:
            r = R.ratio(emu, target, bnd).max().item()
            k = "fp32" if c["c_fp32"] else "bf16"
            worst[k] = max(worst[k], r)
            assert r <= 1.0, (c["name"], r)
    print("worst emulation err / bound:", worst)
    assert worst["bf16"] > 0.5          # the bf16 bound is sharp: a correctly rounded result comes close to it


def _tile_ids(rows, N, tile):
    tm, tn = tile
    return (rows // tm)[:, None] * (-(-N // tn)) + (torch.arange(N) // tn)[None, :]


def test_bounds_catch_injected_faults_in_every_tile(checked):
    """fp32 C: the emulation with its last k index dropped, or with one 8-column group of every column tile shifted by one
    column, breaks the bound on at least one element of every tile."""
    n = 0
    for c, sl in checked:
        if not c["c_fp32"]:
            continue
        for rows, target, bnd, emu, dropped in sl:
            ids = _tile_ids(rows, c["N"], c["tile"])
            every = set(ids.unique().tolist())
            for what, faulty in (("dropped k", dropped), ("shifted column group", R.shift_groups(emu, c["tile"][1]))):
                bad = R.ratio(faulty, target, bnd) > 1.0
                caught = set(ids[bad].unique().tolist())
                assert caught == every, (c["name"], what, sorted(every - caught)[:8])
                n += 1
    assert n > 50


def _sweep_values():
    Ms = {1, 8, 127, 128, 129, 255, 256, 257, 4095, 4096, 8191, 8192}
    for N, K, b in ((768, 192, 0), (1024, 64, 1), (1024, 64, 0)):
        M = R.first_m("160x128", 4096, 4096 + 320 * CUS, N, K, b, 0, 0, CUS)
        assert M is not None
        Ms.update((M - 1, M, M + 1))
    M = R.first_m("phased_persistent", 4096, 4096 + 256 * 512, 2048, 448, 0, 0, 0, CUS)
    assert M is not None
    Ms.update((M - 1, M, M + 1, 131072))
    Ns = {4, 44, 100}
    for step in (96, 128, 192, 256):
        for n in range(step, 3072 + 1, step):
            Ns.update((n, n + 8))
    return sorted(Ms), sorted(Ns), (8, 40, 64, 128, 192, 384, 448, 512, 576, 768)


def test_every_reachable_key_has_a_case(lib):
    have = {c["key"] for c in R.gemm_cases(CUS)}
    Ms, Ns, Ks = _sweep_values()
    reached = {}
    for a, b in ((0, 0), (0, 1), (1, 1)):
        for M in Ms:
            if a and M % 8:
                continue
            for N in Ns:
                if b and N % 8:
                    continue
                for K in Ks:
                    for c32, splits in ((0, 1), (1, 1), (1, 2), (1, 3), (1, 7)):
                        for bias in (0, 1):
                            p = R.plan(M, N, K, a, b, c32, bias, N, splits, CUS)
                            if p is not None:
                                reached.setdefault((p[0], a, b, c32, p[3]), (M, N, K, splits, bias))
    assert len(reached) >= 20
    missing = {k: v for k, v in reached.items() if k not in have}
    assert not missing, missing
    assert have <= set(reached), have - set(reached)             # and no case states a key the sweep cannot reach
    for k in reached:
        assert k[0] not in R.LEFT_OUT, (k, reached[k])             # a retune that opens a left-out key must add its cases


def test_every_reachable_grouped_key_has_a_case(lib):
    have = {k for g in R.grouped_cases() for k in g["keys"]}
    reached = {}
    for Kd in (40, 64, 128, 640, 50048):
        for M in (8, 44, 128, 192, 256, 384, 512, 768, 1024, 1536):
            for N in (8, 40, 128, 192, 256, 384, 512, 768):
                for sp in (1, 2):
                    k = R.grouped_plan([R._p(Kd, M, N, sp)])
                    if k is not None:
                        reached.setdefault(k, (Kd, M, N, sp))
    assert len(reached) == 8, reached          # 128 x 128 with both stagings, 256 x 256 phased or not, four more tile classes
    assert set(reached) == have, (set(reached) - have, have - set(reached))
    for probs in R.GROUPED_REFUSED:
        assert R.grouped_plan(probs) is None


def test_plan_query_refuses_what_the_entry_refuses(lib):
    assert R.plan(128, 128, 64, 1, 0, 1, 0, 128, 1, CUS) is None          # A K-slow with B K-contiguous: not built
    assert R.plan(128, 128, 60, 0, 0, 1, 0, 128, 1, CUS) is None          # contiguous extent not a multiple of 8
    assert R.plan(128, 128, 128, 0, 0, 0, 0, 128, 2, CUS) is None         # split-K partials must be fp32
    assert R.plan(128, 128, 640, 0, 0, 1, 0, 128, 7, CUS) is None         # 640 does not cut into 7 slices of whole tiles
    assert R.plan(128, 126, 64, 0, 0, 1, 0, 126, 1, CUS) is None          # ldc % 4
    assert R.plan(128, 128, 64, 0, 0, 1, 0, 128, 1, CUS) == ("128x128", 128, 128, 1)
    # the CU count is an argument: the per-tile phased form opens on a part with 512 CUs or more, and only there
    assert R.plan(16500, 2048, 448, 0, 0, 0, 0, 2048, 1, 1024)[0] == "phased_tile"
    assert R.plan(16500, 2048, 448, 0, 0, 0, 0, 2048, 1, CUS)[0] == "phased_persistent"
