"""Hierarchical channel sampling on the HIP path (fastvim_amd/hcs.py, the channel embed kernels of csrc/glue.hip,
``SegmentedTrainStep(..., hcs=sampler)``): the kernels against the torch expressions they replace, bit for bit; the model
against the reference golden and the fp64 oracle with a forced subset; the graph-replayed step with one family of graphs
per channel count against the eager step whose model draws inside ``forward``, bit for bit."""
import random
import warnings

import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
F64 = torch.float64


def _err(a, b):
    return (a.double().cpu() - b.double().cpu()).abs().max().item()


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def _sel(channels):
    return None if channels is None else torch.tensor(list(channels), dtype=torch.int32, device="cuda")


def torch_unfold(x, channels, p, colwise, dtype):
    """What PatchEmbedPerChannel ran before the kernel: the gather, the reshape / permute / reshape copy, the cast."""
    if channels is not None:
        x = x[:, channels, :, :]
    B, C, H, W = x.shape
    gh, gw = H // p, W // p
    p6 = x.reshape(B, C, gh, p, gw, p)
    patches = p6.permute(0, 4, 2, 1, 3, 5) if colwise else p6.permute(0, 2, 4, 1, 3, 5)
    return patches.reshape(B, gh * gw * C, p * p).to(dtype)


# ---------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("in_dtype,out_dtype", [(torch.float32, torch.bfloat16), (torch.float32, torch.float32),
                                                (torch.bfloat16, torch.bfloat16)])
@pytest.mark.parametrize("patch", [16, 8])
@pytest.mark.parametrize("colwise", [False, True])
@pytest.mark.parametrize("shape", [(4, 5, 64, 96), (3, 8, 224, 224)])
def test_patch_unfold_chan_bitwise(shape, colwise, patch, in_dtype, out_dtype):
    from fastvim_amd import glue_ops as G
    B, C, H, W = shape
    x = torch.randn(shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(C + patch)).to(in_dtype)
    subsets = [[0], [C - 1], None, [3, 0, 4, 1], list(range(C))[1::2], sorted(set(range(C)) - {2})]
    for channels in subsets:
        n = C if channels is None else len(channels)
        got = G.patch_unfold_chan(x, patch, patch, out_dtype, _sel(channels), n, colwise=colwise)
        want = torch_unfold(x, channels, patch, colwise, out_dtype)
        assert _bits(got, want), (channels, (got.float() - want.float()).abs().max().item())
    # the identity with fewer channels than the image has: the first n
    got = G.patch_unfold_chan(x, patch, patch, out_dtype, None, 2, colwise=colwise)
    assert _bits(got, torch_unfold(x, [0, 1], patch, colwise, out_dtype))


def test_patch_unfold_chan_reads_the_block_when_it_runs():
    """The indices are no launch argument: the same call with a rewritten device array gathers the new channels, and
    an index outside the image is clamped into it instead of read."""
    from fastvim_amd import glue_ops as G
    x = torch.randn(2, 6, 32, 32, device="cuda")
    sel = _sel([1, 4])
    a = G.patch_unfold_chan(x, 16, 16, torch.float32, sel, 2)
    sel.copy_(_sel([5, 0]))
    b = G.patch_unfold_chan(x, 16, 16, torch.float32, sel, 2)
    assert _bits(a, torch_unfold(x, [1, 4], 16, False, torch.float32))
    assert _bits(b, torch_unfold(x, [5, 0], 16, False, torch.float32))
    sel.copy_(_sel([-3, 77]))
    c = G.patch_unfold_chan(x, 16, 16, torch.float32, sel, 2)
    assert _bits(c, torch_unfold(x, [0, 5], 16, False, torch.float32))


def test_chan_embed_table_and_scatter_bitwise():
    from fastvim_amd import glue_ops as G
    g = torch.Generator(device="cuda").manual_seed(3)
    Ctot, D, P = 8, 384, 196
    chan = torch.randn(Ctot, D, device="cuda", generator=g)
    bias = torch.randn(D, device="cuda", generator=g)
    pos = torch.randn(P, D, device="cuda", generator=g)
    for channels in ([5], None, [6, 0, 3], [0, 1, 2, 3, 4, 5, 6]):
        idx = list(range(Ctot)) if channels is None else channels
        n = len(idx)
        for b_, p_ in ((bias, pos), (None, pos), (bias, None), (None, None)):
            want = chan[idx][None]                                       # (1, n, D), broadcast over positions
            if b_ is not None:
                want = want + b_
            if p_ is not None:
                want = want + p_[:, None]
            want = want.expand(P, n, D).reshape(P * n, D)
            got = G.chan_embed_table(chan, b_, p_, _sel(channels), n, P)
            assert _bits(got, want.contiguous()), (channels, b_ is None, p_ is None)
        d_chan = torch.randn(n, D, device="cuda", generator=g)
        base = torch.randn(Ctot, D, device="cuda", generator=g)
        d_table = base.clone()
        G.chan_embed_scatter_(d_table, d_chan, _sel(channels))
        want = base.clone()
        want[idx] += d_chan
        assert _bits(d_table, want)
        rest = [c for c in range(Ctot) if c not in idx]
        assert torch.equal(d_table[rest], base[rest])                    # rows of undrawn channels are not touched


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("with_pos", [True, False])
@pytest.mark.parametrize("channels", [[2], None, [4, 0, 3], [0, 1, 3, 4]])
def test_table_gemm_route_equals_linear_plus_epilogue_bitwise(channels, with_pos, dtype):
    """``_ChanPatchProjFn`` (table + GEMM) against ``LinearFn`` + ``_ChannelEmbedEpilogueFn`` fed the torch-gathered
    embedding: forward and the gradients of proj.weight, proj.bias, pos_embed and channel_embed.weight, bit for bit."""
    from fastvim_amd.mamba_simple_faster import LinearFn
    from fastvim_amd.models_channel_mamba_faster import _ChanPatchProjFn, _ChannelEmbedEpilogueFn
    g = torch.Generator(device="cuda").manual_seed(17)
    Ctot, D, P, B, ph = 5, 64, 24, 8, 16
    idx = list(range(Ctot)) if channels is None else channels
    C = len(idx)
    patches = torch.randn(B, P * C, ph * ph, device="cuda", generator=g).to(dtype)
    gout = torch.randn(B, P * C, D, device="cuda", generator=g)

    def params():
        gg = torch.Generator(device="cuda").manual_seed(5)
        W = (0.05 * torch.randn(D, 1, 1, ph, ph, device="cuda", generator=gg)).requires_grad_()
        bias = torch.randn(D, device="cuda", generator=gg).requires_grad_()
        chan = torch.randn(Ctot, D, device="cuda", generator=gg).requires_grad_()
        pos = torch.randn(1, P, D, device="cuda", generator=gg).requires_grad_() if with_pos else None
        return W, bias, chan, pos

    W1, b1, c1, p1 = params()
    lin = LinearFn.apply(patches, W1, dtype)
    ref = _ChannelEmbedEpilogueFn.apply(lin.view(B, P, C, D), b1, c1[:Ctot][None][:, idx], p1).view(B, P * C, D)
    ref.backward(gout)

    W2, b2, c2, p2 = params()
    out = _ChanPatchProjFn.apply(patches, W2, b2, c2, p2, _sel(channels), C, dtype)
    out.backward(gout)
    assert out.dtype == torch.float32 and _bits(out, ref)
    assert _bits(W2.grad, W1.grad) and _bits(b2.grad, b1.grad) and _bits(c2.grad, c1.grad)
    if with_pos:
        assert _bits(p2.grad, p1.grad)
    rest = [c for c in range(Ctot) if c not in idx]
    assert (c2.grad[rest] == 0).all() and (c2.grad[idx] != 0).any()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("colwise", [False, True])
def test_patch_embed_module_equals_its_copy_chain_bitwise(colwise, dtype):
    """The whole module, kernel path against the strided-copy path it keeps for per-sample channel ids (entered here by
    handing it ``input_channel_order`` = arange, which selects the same embedding rows): tokens, and the gradients of the
    projection weight and the position embedding."""
    from fastvim_amd.models_channel_mamba_faster import PatchEmbedPerChannel
    torch.manual_seed(1)
    pe = PatchEmbedPerChannel(img_size=(64, 96), patch_size=16, stride=16, in_chans=5, embed_dim=64, hcs=False,
                              scanpath_type="colwise" if colwise else "rowwise").cuda()
    pos = torch.randn(1, pe.num_patches, 64, device="cuda").requires_grad_()
    x = torch.randn(4, 5, 64, 96, device="cuda")
    order = torch.arange(5, device="cuda")[None].expand(4, 5)
    outs = []
    for kw in ({}, {"input_channel_order": order}):
        pe.zero_grad(set_to_none=True)
        pos.grad = None
        with torch.autocast("cuda", dtype=dtype, enabled=dtype != torch.float32):
            out = pe(x, pos_embed=pos, **kw)[0]
        out.square().sum().backward()
        # (not the bias / channel rows: with per-sample ids the copy chain sums those per sample first, another order)
        outs.append((out.detach(), pe.proj.weight.grad.clone(), pos.grad.clone()))
    for a, b in zip(*outs):
        assert _bits(a, b)


# ---------------------------------------------------------------------------------------------- model
def test_channel_model_with_sampler_vs_reference_golden():
    """``tiny_64x96_c5_hcs`` with the sampler set to the subset the reference drew: same tolerances as
    test_channel_gpu.py::test_channel_model_vs_reference_golden, and the forward leaves Python's RNG alone."""
    from fastvim_amd.hcs import ChannelSampler
    from fastvim_amd.models_channel_mamba_faster import VisionMamba
    c = load_golden("channel.pt")["tiny_64x96_c5_hcs"]
    m = VisionMamba(img_size=c["img"], patch_size=16, depth=4, embed_dim=32, channels=c["channels"],
                    num_classes=10, rms_norm=True, residual_in_fp32=True, fused_add_norm=True,
                    final_pool_type="mean", if_abs_pos_embed=True, drop_path_rate=0.0).cuda()
    m.load_state_dict(c["state_dict"], strict=True)
    m.train(c["train"])
    assert c["train"]
    sampler = ChannelSampler(c["channels"])
    sampler.set(c["subset"])
    random.seed(99)
    state = random.getstate()
    logits = m(c["x"].cuda(), hcs=sampler)
    assert random.getstate() == state
    assert m._tokens_per_patch == len(c["subset"])
    ref = c["logits"]
    assert _err(logits, ref) <= 2e-5 * max(1.0, ref.abs().max().item()), _err(logits, ref)
    logits.backward(c["g"].cuda())
    params = dict(m.named_parameters())
    for k, gref in c["grads"].items():
        e = _err(params[k].grad, gref)
        assert e <= 2e-4 * max(1.0, gref.abs().max().item()), (k, e, gref.abs().max().item())
    # the same forward without the sampler, drawing for itself: the same subset under the golden's seed, the same logits
    random.seed(c["py_seed"])
    assert _bits(m(c["x"].cuda()), logits)


@pytest.mark.parametrize("subset", [[1, 4, 6], [0, 1, 2, 3, 4, 5, 6]])
def test_channelvim_small_config5_width_with_subset_vs_oracle(subset):
    """FastChannelVim-S/16 width, 8 channels, 224 px, depth 3, a drawn subset: tolerances of
    test_channel_gpu.py::test_channelvim_small_config5_shape_vs_oracle."""
    from fastvim_amd.hcs import ChannelSampler
    from fastvim_amd.models_channel_mamba_faster import VisionMamba
    from oracle import channel_forward_oracle, make_channel_state_dict
    sd = make_channel_state_dict(seed=5, embed_dim=384, depth=3, channels=8, num_classes=16)
    m = VisionMamba(img_size=224, depth=3, embed_dim=384, channels=8, num_classes=16, rms_norm=True,
                    residual_in_fp32=True, fused_add_norm=True, hcs=True, drop_path_rate=0.0).cuda().train()
    m.load_state_dict(sd, strict=True)
    x = torch.randn(2, 8, 224, 224, generator=torch.Generator().manual_seed(9))
    g = torch.randn(2, 16, generator=torch.Generator().manual_seed(10))
    p = {k: v.clone().requires_grad_() for k, v in sd.items()}
    ref = channel_forward_oracle(p, x, depth=3, compute_dtype=F64, channels=subset)
    ref.backward(g.double())
    sampler = ChannelSampler(8)
    sampler.set(subset)
    logits = m(x.cuda(), hcs=sampler)
    s = max(1.0, ref.abs().max().item())
    assert _err(logits, ref) <= 5e-5 * s, _err(logits, ref)
    logits.backward(g.cuda())
    for n, q in m.named_parameters():
        gr = p[n].grad
        e = _err(q.grad, gr)
        assert e <= 5e-4 * max(1.0, gr.abs().max().item()), (n, e, gr.abs().max().item())
    rest = [c for c in range(8) if c not in subset]
    assert (m.patch_embed.channel_embed.weight.grad[rest] == 0).all()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        lb = m(x.cuda(), hcs=sampler)
    assert _err(lb, ref) <= 5e-2 * s, _err(lb, ref)


# ---------------------------------------------------------------------------------------------- the replayed step
B_, NCLS = 8, 10


def _make(drop_path=0.1, depth=6, hcs=True):
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    from fastvim_amd.models_channel_mamba_faster import VisionMamba
    torch.manual_seed(0)
    m = VisionMamba(img_size=64, patch_size=16, depth=depth, embed_dim=192, channels=8, num_classes=NCLS, rms_norm=True,
                    residual_in_fp32=True, fused_add_norm=True, final_pool_type="mean", if_abs_pos_embed=True,
                    drop_path_rate=drop_path, hcs=hcs).cuda().train()
    flat = FlatTrainingState(m)
    nd = {n for n, p in m.named_parameters() if p.ndim <= 1 or n.endswith(".bias") or n in m.no_weight_decay()
          or getattr(p, "_no_weight_decay", False)}
    return m, flat, FlatAdamW(flat, m, lr=1e-3, weight_decay=0.05, no_decay=nd, ema_decay=0.999)


def _batches(n=3):
    g = torch.Generator(device="cuda").manual_seed(11)
    return [(torch.randn(B_, 8, 64, 64, device="cuda", generator=g), torch.randint(0, NCLS, (B_,), device="cuda", generator=g))
            for _ in range(n)]


def _same_state(f1, o1, f2, o2):
    assert torch.equal(f1.param_flat, f2.param_flat)
    assert torch.equal(o1.exp_avg, o2.exp_avg) and torch.equal(o1.exp_avg_sq, o2.exp_avg_sq)
    assert torch.equal(o1.ema, o2.ema)


def test_graph_step_with_sampler_equals_eager_step_drawing_in_forward():
    """The real recipe, trajectory against trajectory.  Reference: the eager step whose model draws inside ``forward``
    (what runs without this feature).  Under test: graph replay, ``sampler.sample(); step()``.  Same ``random.seed``: the
    same stream of subsets; losses, parameters, Adam moments and EMA bit-identical.  The run goes on until every count
    1..8 has occurred (asserted from the sampler's own record; at most 40 steps), which interleaves the eight families of
    graphs that share one memory pool."""
    from fastvim_amd.hcs import ChannelSampler
    from fastvim_amd.pipeline import SegmentedTrainStep
    batches = _batches()
    loss_fn = torch.nn.CrossEntropyLoss()

    # under test first: its record of draws fixes the number of steps
    m2, f2, o2 = _make()
    sampler = ChannelSampler(8)
    sampler.set([2, 5, 7])
    x2 = torch.zeros(B_, 8, 64, 64, device="cuda")
    y2 = torch.zeros(B_, dtype=torch.int64, device="cuda")
    torch.manual_seed(7)
    random.seed(2)
    py_state = random.getstate()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        step = SegmentedTrainStep(m2, f2, o2, loss_fn, x2, y2, n_segments=3, use_graph=True, warmup=2, hcs=sampler)
    assert not [w for w in rec if "frozen" in str(w.message)]                 # with a sampler there is nothing to warn about
    assert step.use_graph
    assert sampler.last() == [2, 5, 7] and random.getstate() == py_state      # construction leaves sampler and RNG alone
    assert o2.step_t.item() == 0.0
    assert sorted(step.families) == list(range(1, 9))                         # eight families ...
    fwd_graphs = {id(fam[0]) for fam in step.families.values()}
    assert len(fwd_graphs) == 8 and all(len(fam[1]) == step.K for fam in step.families.values())
    assert isinstance(step.graphs[2], torch.cuda.CUDAGraph)                   # ... and one optimizer graph
    got, draws = [], []
    while len(got) < 12 or (len({len(d) for d in draws}) < 8 and len(got) < 40):
        xb, yb = batches[len(got) % len(batches)]
        x2.copy_(xb)
        y2.copy_(yb)
        draws.append(sampler.sample())
        assert sampler.count == len(draws[-1])
        got.append(step.step().item())
    torch.cuda.synchronize()
    assert {len(d) for d in draws} == set(range(1, 9)), [len(d) for d in draws]
    n_steps = len(got)

    m1, f1, o1 = _make()
    x1 = torch.zeros(B_, 8, 64, 64, device="cuda")
    y1 = torch.zeros(B_, dtype=torch.int64, device="cuda")
    torch.manual_seed(7)
    random.seed(2)
    ref_step = SegmentedTrainStep(m1, f1, o1, loss_fn, x1, y1, n_segments=3, use_graph=False)
    ref, ref_counts = [], []
    for i in range(n_steps):
        xb, yb = batches[i % len(batches)]
        x1.copy_(xb)
        y1.copy_(yb)
        ref.append(ref_step.step().item())
        ref_counts.append(m1._tokens_per_patch)
    torch.cuda.synchronize()
    assert ref_counts == [len(d) for d in draws]
    assert got == ref, (got, ref)
    assert all(v == v for v in got)
    assert o2.step_t.item() == float(n_steps) == o1.step_t.item() and n_steps >= 12
    _same_state(f1, o1, f2, o2)
    f1.close(); f2.close()


def test_replays_read_the_index_array():
    """Two replays of the SAME family with two subsets: each equals the eager step on that subset, and they differ."""
    from fastvim_amd.hcs import ChannelSampler
    from fastvim_amd.pipeline import SegmentedTrainStep
    (xb, yb), = _batches(1)
    loss_fn = torch.nn.CrossEntropyLoss()
    seq = [[0, 1], [6, 7]]
    runs = []
    for use_graph in (False, True):
        m, f, o = _make(drop_path=0.0, depth=3)
        sampler = ChannelSampler(8)
        x = xb.clone()
        y = yb.clone()
        step = SegmentedTrainStep(m, f, o, loss_fn, x, y, n_segments=3, use_graph=use_graph, warmup=2, hcs=sampler)
        assert step.use_graph is use_graph
        losses = []
        for s in seq:
            sampler.set(s)
            losses.append(step.step().item())
        torch.cuda.synchronize()
        runs.append((losses, f, o))
    (l1, f1, o1), (l2, f2, o2) = runs
    assert l1 == l2 and l1[0] != l1[1], (l1, l2)
    _same_state(f1, o1, f2, o2)
    f1.close(); f2.close()


def test_graph_step_with_mixup_and_sampler_equals_eager_composition():
    """``mixup=`` and ``hcs=`` together, four steps: the replayed step against the eager composition of the same pieces (the
    full image is mixed by fv_mix_batch, then the channels are selected -- the reference's order)."""
    from fastvim_amd.hcs import ChannelSampler
    from fastvim_amd.mixup import Mixup
    from fastvim_amd.pipeline import SegmentedTrainStep
    batches = _batches(2)
    seq = [((0.3172, False, None), [1, 3, 4]), ((0.71, True, (10, 50, 0, 37)), [0, 2, 3, 4, 5, 6, 7]),
           ((1.0, False, None), [5]), ((0.55, True, (20, 64, 30, 64)), [1, 3, 4])]
    runs = []
    for use_graph in (False, True):
        m, f, o = _make()
        sampler = ChannelSampler(8)
        mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=NCLS)
        mix.set(0.5)
        x = torch.zeros(B_, 8, 64, 64, device="cuda")
        y = torch.zeros(B_, dtype=torch.int64, device="cuda")
        torch.manual_seed(7)
        step = SegmentedTrainStep(m, f, o, mix.criterion(), x, y, n_segments=3, use_graph=use_graph, warmup=2, mixup=mix,
                                  hcs=sampler)
        assert step.use_graph is use_graph and step._x_mixed is not None
        losses = []
        for i, ((lam, cut, box), subset) in enumerate(seq):
            xb, yb = batches[i % 2]
            x.copy_(xb)
            y.copy_(yb)
            mix.set(lam, use_cutmix=cut, box=box)
            sampler.set(subset)
            losses.append(step.step().item())
        torch.cuda.synchronize()
        assert torch.equal(x, batches[(len(seq) - 1) % 2][0])                 # the input buffer is never written
        runs.append((losses, f, o))
    (l1, f1, o1), (l2, f2, o2) = runs
    assert l1 == l2 and len(set(l1)) == len(l1) and all(v == v for v in l1), (l1, l2)
    _same_state(f1, o1, f2, o2)
    f1.close(); f2.close()


# ---------------------------------------------------------------------------------------------- error paths
def test_sampler_with_input_channel_order_is_refused():
    from fastvim_amd.hcs import ChannelSampler
    from fastvim_amd.models_channel_mamba_faster import PatchEmbedPerChannel
    pe = PatchEmbedPerChannel(img_size=32, patch_size=16, stride=16, in_chans=4, embed_dim=32).cuda().train()
    x = torch.randn(2, 4, 32, 32, device="cuda")
    order = torch.arange(4, device="cuda")[None].expand(2, 4)
    with pytest.raises(NotImplementedError):
        pe(x, input_channel_order=order, hcs=ChannelSampler(4))
    with pytest.raises(ValueError):
        pe(x, hcs=ChannelSampler(5))                         # a sampler for another channel count


def test_step_refuses_a_model_whose_embed_lacks_the_keyword():
    from fastvim_amd.hcs import ChannelSampler
    from fastvim_amd.pipeline import SegmentedTrainStep

    class NoKeyword(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def _embed(self, x):
            return self.inner._embed(x)

        def __getattr__(self, name):
            try:
                return super().__getattr__(name)
            except AttributeError:
                return getattr(super().__getattr__("inner"), name)

    m, f, o = _make(depth=3)
    x = torch.zeros(B_, 8, 64, 64, device="cuda")
    y = torch.zeros(B_, dtype=torch.int64, device="cuda")
    with pytest.raises(TypeError):
        SegmentedTrainStep(NoKeyword(m), f, o, torch.nn.CrossEntropyLoss(), x, y, use_graph=False, hcs=ChannelSampler(8))
    f.close()


def test_capture_without_sampler_warns_once_that_the_subset_is_frozen():
    from fastvim_amd.pipeline import SegmentedTrainStep
    m, f, o = _make(drop_path=0.0, depth=3)
    (xb, yb), = _batches(1)
    random.seed(4)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        step = SegmentedTrainStep(m, f, o, torch.nn.CrossEntropyLoss(), xb.clone(), yb.clone(), n_segments=3, use_graph=True, warmup=2)
    frozen = [w for w in rec if issubclass(w.category, RuntimeWarning) and "frozen" in str(w.message)]
    assert step.use_graph and len(frozen) == 1, [str(w.message) for w in rec]
    frozen_count = m._tokens_per_patch
    a = step.step().item()
    b = step.step().item()
    torch.cuda.synchronize()
    assert a == a and b == b and m._tokens_per_patch == frozen_count          # (it replays: the announced behaviour)
    f.close()
    # hcs off, or eval: nothing is sampled, nothing to announce
    m2, f2, o2 = _make(drop_path=0.0, depth=3, hcs=False)
    m2.eval()
    with warnings.catch_warnings(record=True) as rec2:
        warnings.simplefilter("always")
        SegmentedTrainStep(m2, f2, o2, torch.nn.CrossEntropyLoss(), xb.clone(), yb.clone(), n_segments=3, use_graph=False)
    assert not [w for w in rec2 if "frozen" in str(w.message)]
    f2.close()


def test_eval_uses_every_channel_and_draws_as_before():
    """Eval mode with a sampler given: identity selection, and the ``random.sample`` of :184-185 is consumed as ever."""
    from fastvim_amd.hcs import ChannelSampler
    from fastvim_amd.models_channel_mamba_faster import VisionMamba
    torch.manual_seed(0)
    m = VisionMamba(img_size=64, depth=2, embed_dim=64, channels=5, num_classes=10, rms_norm=True, residual_in_fp32=True,
                    fused_add_norm=True, final_pool_type="mean", if_abs_pos_embed=True).cuda().eval()
    x = torch.randn(2, 5, 64, 64, device="cuda")
    sampler = ChannelSampler(5)
    sampler.set([1, 3])
    with torch.no_grad():
        random.seed(8)
        a, _ = m._embed(x, hcs=sampler)
        state_a = random.getstate()
        assert m._tokens_per_patch == 5
        random.seed(8)
        b, _ = m._embed(x)
        state_b = random.getstate()
        random.seed(8)
        random.sample(range(5), k=5)
        assert state_a == state_b == random.getstate()
        m.train()
        c, _ = m._embed(x, hcs=sampler)
        assert m._tokens_per_patch == 2 and c.shape[1] == 2 * m.num_patches
    assert _bits(a, b) and a.shape[1] == 5 * m.num_patches
    assert sampler.last() == [1, 3]
