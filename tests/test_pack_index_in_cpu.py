"""The fragment-major layout of in_proj.weight as the operand of its forward product (mixer_ops.pack_index_in): a permutation
of the weight's 16-byte units, and the map the header and the pack kernel state."""
import torch


def test_pack_index_in_is_a_permutation_and_equals_the_formula():
    from fastvim_amd.mixer_ops import PACK_IN_K, pack_index_in, pack_weight_frags_in_ref
    N, K = 768, 192
    assert PACK_IN_K == K
    idx = pack_index_in(N)
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (N * K // 8, 2)
    # every 16-byte unit of the weight exactly once
    flat = idx[:, 0] * (K // 8) + idx[:, 1] // 8
    assert (idx[:, 1] % 8 == 0).all() and (idx[:, 0] >= 0).all() and (idx[:, 0] < N).all() and (idx[:, 1] < K).all()
    assert torch.equal(torch.sort(flat).values, torch.arange(N * K // 8))
    # unit (((p * 4 + wv) * 6 + ks) * 6 + nb) * 64 + lane = W[384 p + 96 wv + 16 nb + (lane & 15)][32 ks + 8 (lane >> 4) .. + 8)
    u = 0
    for p in range(N // 384):
        for wv in range(4):
            for ks in range(6):
                for nb in range(6):
                    lane = torch.arange(64)
                    want = torch.stack([384 * p + 96 * wv + 16 * nb + (lane & 15), 32 * ks + 8 * (lane >> 4)], dim=1)
                    assert torch.equal(idx[u:u + 64], want), (p, wv, ks, nb)
                    u += 64
    assert u == N * K // 8
    # the gather built on it moves whole units
    W = torch.arange(N * K, dtype=torch.int32).reshape(N, K)
    pk = pack_weight_frags_in_ref(W).reshape(-1, 8)
    assert torch.equal(pk[:, 0], idx[:, 0].int() * K + idx[:, 1].int())
    assert torch.equal(pk, pk[:, :1] + torch.arange(8, dtype=torch.int32))


def test_pack_index_in_other_widths():
    from fastvim_amd.mixer_ops import pack_index_in
    for N in (384, 1152):
        idx = pack_index_in(N)
        flat = idx[:, 0] * 24 + idx[:, 1] // 8
        assert torch.equal(torch.sort(flat).values, torch.arange(N * 24))
