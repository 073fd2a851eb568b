"""The fragment-major layout of out_proj.weight as the K-slow operand of its data gradient (mixer_ops.pack_index_w2),
checked on the CPU against the formula the kernels use -- no GPU needed."""
import torch


def test_pack_index_w2_is_the_formula_and_a_bijection():
    from fastvim_amd.mixer_ops import pack_index_w2
    idx = pack_index_w2()
    assert idx.shape == (192 * 384 // 8, 8, 2)
    for u in (0, 1, 15, 16, 63, 64, 383, 384, 2303, 2304, 4607, 9215):
        lane, t = u % 64, u // 64
        nb, ks, wv = t % 6, (t // 6) % 6, t // 36
        for j in range(8):
            assert idx[u, j].tolist() == [32 * ks + 8 * (lane // 16) + j, 96 * wv + 16 * nb + (lane % 16)]
    flat = (idx[..., 0] * 384 + idx[..., 1]).reshape(-1)
    assert flat.min() == 0 and flat.max() == 192 * 384 - 1
    assert torch.equal(torch.sort(flat).values, torch.arange(192 * 384))          # every element exactly once
    # a wave's stream is one run: wave wv's units are [wv * 2304, (wv + 1) * 2304) and hold columns [96 wv, 96 wv + 96) only
    for wv in range(4):
        cols = idx[wv * 2304:(wv + 1) * 2304, :, 1]
        assert cols.min() == 96 * wv and cols.max() == 96 * wv + 95


def test_pack_weight_frags_w2_ref_moves_every_element():
    from fastvim_amd.mixer_ops import pack_index_w2, pack_weight_frags_w2_ref
    W = torch.arange(192 * 384, dtype=torch.int32).reshape(192, 384)
    P = pack_weight_frags_w2_ref(W)
    assert P.shape == W.shape
    idx = pack_index_w2()
    assert torch.equal(P.reshape(-1, 8), idx[..., 0].to(torch.int32) * 384 + idx[..., 1].to(torch.int32))
