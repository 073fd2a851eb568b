"""Pure-torch restatement of the MAE token plan (csrc/mae_tokens.hip, fastvim_amd/mae_tokens.py) and of the decoder's input
assembly, for the CPU and GPU tests: ``argsort(stable=True)``, index arithmetic and ``torch.gather`` only."""
import torch

PLAN_KEYS = ("ids_keep", "ids_restore", "mask", "keep_index", "restore_index", "row_index_even", "ids_keep_odd", "order",
             "inverse", "order_index", "inverse_index", "row_index_odd")

GRIDS = ((4, 4), (14, 14), (16, 16), (32, 32))
RATIOS = (0.5, 0.75, 0.9)


def tie_free_noise(B, L, seed):
    """(B, L) fp32, a permutation of (k + 0.5) / L per sample: no two values of a sample are equal."""
    g = torch.Generator().manual_seed(seed)
    return torch.stack([(torch.randperm(L, generator=g).float() + 0.5) / L for _ in range(B)])


def quantised_noise(B, L, seed, levels=8):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, levels, (B, L), generator=g).float() / levels


def plan_ref(noise, H, W, K):
    """The plan of ``noise`` (B, L = H W): dict of the twelve tensors of ``TokenPlan``."""
    B, L = noise.shape
    assert L == H * W
    shuffle = torch.argsort(noise, dim=1, stable=True)                  # rank -> token
    rank = torch.argsort(shuffle, dim=1, stable=True)                   # token -> rank
    ids_keep = shuffle[:, :K].sort(dim=1).values                        # kept tokens, ascending
    kept = rank < K
    place = torch.cumsum(kept.long(), dim=1) - 1                        # a kept token's place among the kept ones
    ids_restore = torch.where(kept, place, rank)
    mask = (~kept).float()
    r = ids_keep // W
    row_even = torch.stack([r, (H - 1) - r.flip(1)]).to(torch.int32)
    key = (ids_keep % W) * H + ids_keep // W                            # place in the transposed grid
    order = torch.argsort(key, dim=1, stable=True)
    ids_keep_odd = torch.gather(key, 1, order)
    inverse = torch.argsort(order, dim=1, stable=True)
    ro = ids_keep_odd // H
    row_odd = torch.stack([ro, (W - 1) - ro.flip(1)]).to(torch.int32)
    return {"ids_keep": ids_keep, "ids_restore": ids_restore, "mask": mask, "keep_index": ids_keep.to(torch.int32),
            "restore_index": torch.where(kept, place, torch.full_like(place, -1)).to(torch.int32), "row_index_even": row_even,
            "ids_keep_odd": ids_keep_odd, "order": order, "inverse": inverse, "order_index": order.to(torch.int32),
            "inverse_index": inverse.to(torch.int32), "row_index_odd": row_odd}


def eager_plan(noise, H, W, K):
    """Today's composition, line for line: ``random_masking``'s index code, ``Block_masked``'s sort / argsort on the
    transposed ids, the masked mixer's div / flip / stack for both layer parities."""
    N, L = noise.shape
    ids_shuffle = torch.argsort(noise, dim=1)
    ids_shuffle[:, :K] = ids_shuffle[:, :K].sort().values
    ids_shuffle = ids_shuffle.contiguous()
    ids_restore = torch.argsort(ids_shuffle, dim=1)
    ids_keep = ids_shuffle[:, :K]
    mask = torch.ones([N, L])
    mask[:, :K] = 0
    mask = torch.gather(mask, dim=1, index=ids_restore)

    def mixer_index(ids, rows, cols):
        r = torch.div(ids, cols, rounding_mode="floor").to(torch.int32)
        return torch.stack([r, (rows - 1) - r.flip(1)]).contiguous()

    indices = torch.arange(H * W, dtype=torch.long)
    rotate_indices = (indices % W) * H + indices.div(W, rounding_mode="floor")
    ids_odd, order = torch.sort(rotate_indices[ids_keep], dim=1)
    inverse = torch.argsort(order, 1)
    return {"ids_keep": ids_keep, "ids_restore": ids_restore, "mask": mask, "row_index_even": mixer_index(ids_keep, H, W),
            "ids_keep_odd": ids_odd, "order": order, "inverse": inverse, "row_index_odd": mixer_index(ids_odd, W, H)}


def decoder_eager(x, mask_token, pos_embed, ids_restore):
    """``forward_decoder``'s chain, as written there."""
    mask_tokens = mask_token.repeat(x.shape[0], ids_restore.shape[1] - x.shape[1], 1)
    x = torch.cat([x, mask_tokens.to(x.dtype)], dim=1)
    x = torch.gather(x, dim=1, index=ids_restore.unsqueeze(-1).repeat(1, 1, x.shape[2]))
    return x + pos_embed


def decoder_mask_token_terms(dout, mask, x_dtype):
    """The terms whose sum is d mask_token, as autograd forms them: the removed rows of ``dout``, rounded to ``x``'s dtype.
    -> (n_removed, D) fp64."""
    rows = dout[mask.bool()]
    return rows.to(x_dtype).double()
