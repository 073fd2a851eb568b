"""The fragment-major weight layout of the packed projection launches (mixer_ops.pack_index), checked on the CPU against
its definition: for a weight Wk (192, K), K contiguous, KS = K / 32, the 16-byte unit

    u = ((wv * KS + ks) * 3 + nb) * 64 + lane        wv 0..3, ks 0..KS-1, nb 0..2, lane 0..63

holds Wk[48 wv + 16 nb + (lane & 15)][32 ks + 8 (lane >> 4) .. + 8)."""
import pytest
import torch


@pytest.mark.parametrize("K", [384, 768])
def test_pack_index_is_the_formula_and_a_bijection(K):
    from fastvim_amd.mixer_ops import pack_index
    idx = pack_index(K)
    KS = K // 32
    n_units = 192 * K // 8
    assert tuple(idx.shape) == (n_units, 2) and idx.dtype == torch.int64
    seen = set()
    for wv in range(4):
        for ks in range(KS):
            for nb in range(3):
                for lane in range(64):
                    u = ((wv * KS + ks) * 3 + nb) * 64 + lane
                    row, col = 48 * wv + 16 * nb + (lane & 15), 32 * ks + 8 * (lane >> 4)
                    assert idx[u, 0].item() == row and idx[u, 1].item() == col, (wv, ks, nb, lane)
                    seen.add((row, col))
    # every 8-element unit of the (192, K) weight exactly once
    assert len(seen) == n_units
    assert seen == {(r, c) for r in range(192) for c in range(0, K, 8)}


@pytest.mark.parametrize("K", [384, 768])
def test_pack_reference_is_a_permutation_in_16_byte_units(K):
    from fastvim_amd.mixer_ops import pack_index, pack_weight_frags_ref
    W = torch.arange(192 * K, dtype=torch.int32).reshape(192, K)
    P = pack_weight_frags_ref(W)
    assert P.shape == W.shape
    flat = P.reshape(-1, 8)
    idx = pack_index(K)
    assert torch.equal(flat[:, 0].long(), idx[:, 0] * K + idx[:, 1])                     # a unit starts where the map says ...
    assert torch.equal(flat, flat[:, :1] + torch.arange(8, dtype=torch.int32))           # ... and is 8 consecutive elements
    assert torch.equal(P.reshape(-1).sort().values, W.reshape(-1))
    # a wave instruction (64 lanes of one (wv, ks, nb)) is 1 KiB contiguous, a wave's whole stream one run of 192 * K / 4 elements
    quarter = 192 * K // 4
    for wv in range(4):
        rows = idx[wv * quarter // 8:(wv + 1) * quarter // 8, 0]
        assert rows.min().item() == 48 * wv and rows.max().item() == 48 * wv + 47
