"""Measure the MAE pre-training step of the Vim baseline (fastvim_amd/mae_step.py: ``VimMAEPretrainStep``) and its class-token
assembly (csrc/mae_tokens_cls.hip) on the GPU, in ONE process, rounds alternating between the variants:

  (a) ``mae_vim_base_dec512d2b`` at 224 px, batch 128, bf16, mask ratio 0.75, as an EAGER loop with ``fused_tokens`` off and
      ``torch.rand`` masks -- the code this model ran before it had a step object;
  (b) the same eager loop with a ``MaskSampler`` (the keyed plan and the two class-token launches, no graphs);
  (c) ``VimMAEPretrainStep(accum_iter=1, n_segments=3)``: a timed call is ``sampler.sample(); step.micro_step()``;
  (d) (a) and (c) with ``accum_iter = 2``, reported per micro-batch;
  (e) stand-alone on HBM-cold rotated operands at (128, 14 x 14, K = 49) with D = 768 and 512, bf16 tokens: each of the four
      launches next to the torch chain it replaces -- the forward chain as the model writes it, the backward chain as the
      plain ops autograd runs behind it, written out (nothing here differentiates: no autograd under the timing capture) --
      and next to a plain copy of the same bytes (``floor_ratio`` as in bench.py).

    python tools/bench_vim_mae_step.py            # --no-step / --no-kernels skip a part

Every GPU phase runs under its own time limit (a watchdog ends the process when a phase overruns: nothing else is then
started on the device).  The log goes to stdout and to ``--log`` (profiles/vim_mae_step_bench.log), the last line one JSON
record.  Sets no threshold."""
import argparse
import json
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))

from bench_mae_tokens import phase, timed  # noqa: E402

FACTORY, IMG = "mae_vim_base_dec512d2b", 224
KERNEL_SHAPES = ((128, 14, 14, 49, 768), (128, 14, 14, 49, 512))        # (B, H, W, K, D): the encoder's and the decoder's width


def _state(batch):
    import torch
    from fastvim_amd import fastvim_mae
    from fastvim_amd.flat import FlatAdamW, FlatTrainingState
    torch.manual_seed(1234)
    model = getattr(fastvim_mae, FACTORY)(img_size=IMG, fused_loss=True).cuda().train()
    x = torch.randn(batch, 3, IMG, IMG, generator=torch.Generator().manual_seed(100)).cuda()
    flat = FlatTrainingState(model)
    no_decay = {n for n, p in model.named_parameters()
                if p.ndim <= 1 or n.endswith(".bias") or n in model.no_weight_decay() or getattr(p, "_no_weight_decay", False)}
    opt = FlatAdamW(flat, model, lr=1.5e-4 * batch / 256, betas=(0.9, 0.95), weight_decay=0.05, no_decay=no_decay, ema_decay=0.9999)
    torch.manual_seed(5678)
    return model, x, flat, opt


def eager_loop(batch, accum_iter, with_sampler):
    """The plain loop: returns (call = one micro-batch, loss of the last call, flat, keep-alive)."""
    import torch
    from fastvim_amd.mae_tokens import MaskSampler
    model, x, flat, opt = _state(batch)
    sampler = MaskSampler(seed=0) if with_sampler else None
    state = {"micro": 0, "loss": None}

    def call():
        if sampler is not None:
            sampler.sample()
        if state["micro"] == 0:
            flat.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = model(x, mask_ratio=0.75, sampler=sampler)[0] if sampler is not None else model(x, mask_ratio=0.75)[0]
        loss.backward()
        flat.finish_backward()
        state["loss"] = loss.detach()
        state["micro"] += 1
        if state["micro"] == accum_iter:
            opt.step(grad_scale=1.0 / accum_iter)
            state["micro"] = 0

    return call, (lambda: state["loss"].item()), flat, (model, opt, x, sampler)


def step_object(batch, accum_iter, n_segments):
    from fastvim_amd.mae_step import VimMAEPretrainStep
    from fastvim_amd.mae_tokens import MaskSampler
    model, x, flat, opt = _state(batch)
    sampler = MaskSampler(seed=0)
    step = VimMAEPretrainStep(model, flat, opt, x, sampler, mask_ratio=0.75, accum_iter=accum_iter, n_segments=n_segments)
    if not step.use_graph:
        raise SystemExit("bench_vim_mae_step.py: the step fell back to eager execution (see its warning)")

    def call():
        sampler.sample()
        step.micro_step()

    return call, (lambda: step.loss.item()), flat, (step, model, opt, x, sampler)


def steps_part(batch, rounds, steps, say):
    variants = (("(a) eager loop, fused_tokens off, torch.rand", lambda: eager_loop(batch, 1, False)),
                ("(b) eager loop, sampler (new launches)", lambda: eager_loop(batch, 1, True)),
                ("(c) VimMAEPretrainStep accum 1, 3 segments", lambda: step_object(batch, 1, 3)),
                ("(d) eager loop, off, accum 2", lambda: eager_loop(batch, 2, False)),
                ("(d) VimMAEPretrainStep accum 2, 3 segments", lambda: step_object(batch, 2, 3)))
    built = {}
    with phase(f"Vim MAE-B {IMG} px, batch {batch}, bf16: build + capture x {len(variants)}", 900, say):
        for name, make in variants:
            built[name] = make()
            for _ in range(4):
                built[name][0]()
    steps = 2 * max(1, steps // 2)                       # whole groups of the accum 2 variants
    ts = {name: [] for name, _ in variants}
    with phase(f"{rounds} alternating rounds of {steps} calls (micro-batches)", 600, say):
        for _ in range(rounds):
            for name, _ in variants:
                ts[name].append(timed(built[name][0], steps))
    rec = {"batch": batch, "calls_per_round": steps}
    for name, _ in variants:
        t = ts[name]
        med = statistics.median(t)
        say(f"    {name:<46} median {med:.3f} ms per micro-batch (min {min(t):.3f}, max {max(t):.3f}) = {batch / med * 1e3:.0f} "
            f"img/s; loss {built[name][1]():.6f}")
        rec[name] = {"ms_per_micro_batch": round(med, 3), "ms_rounds": [round(v, 3) for v in t]}
    names = [n for n, _ in variants]
    for eager, step in ((names[0], names[2]), (names[3], names[4])):
        r = statistics.median(ts[eager]) / statistics.median(ts[step])
        say(f"    {step} runs a micro-batch in 1 / {r:.2f} of the time of {eager}")
        rec[step]["eager_over_step"] = round(r, 3)
    for name, _ in variants:
        built[name][2].close()
    return rec


def kernel_rows(B, H, W, K, D, curve, say):
    import torch
    from bench import floor_us, rotating, time_kernel
    from fastvim_amd import _lib as L
    from fastvim_amd import mae_tokens as MT
    Ln = H * W
    g = torch.Generator().manual_seed(0)
    plan = MT.mask_plan(torch.rand(B, Ln, generator=g).cuda(), (H, W), K)
    bf = torch.bfloat16
    T = {"full": torch.randn(B, Ln, D, generator=g).to(bf).cuda(), "kept1": torch.randn(B, K + 1, D, generator=g).to(bf).cuda(),
         "dkept1": torch.randn(B, K + 1, D, generator=g).to(bf).cuda(),
         "dgrid1": torch.randn(B, Ln + 1, D, generator=g).cuda()}
    vec = torch.randn(1, 1, D, generator=g).cuda()                              # cls_token / mask_token
    pos = torch.randn(1, Ln + 1, D, generator=g).cuda()
    nblocks = -(-(B * (Ln + 1)) // MT.DECODER_ROWS_PER_BLOCK)
    partials = torch.empty(nblocks, D, device="cuda", dtype=torch.float64)
    dvec = torch.empty(D, device="cuda")
    dfull = torch.empty(B, Ln, D, device="cuda", dtype=bf)
    dkept = torch.empty(B, K + 1, D, device="cuda", dtype=bf)
    lib, i32, p_ = L.lib(), L.i32, L.ptr

    def enc_bwd(s):
        rc = lib.fv_mae_encoder_tokens_cls_bwd(p_(s["dkept1"]), p_(plan.restore_index), p_(dfull), i32(L.FV_BF16), p_(dvec), i32(B),
                                               i32(Ln), i32(K), i32(D), L.stream_of(dfull))
        L.check(rc, "mae_encoder_tokens_cls_bwd")

    def dec_bwd(s):
        rc = lib.fv_mae_decoder_tokens_cls_bwd(p_(s["dgrid1"]), p_(plan.restore_index), p_(dkept), i32(L.FV_BF16), p_(partials),
                                               i32(nblocks), p_(dvec), i32(B), i32(Ln), i32(K), i32(D), L.stream_of(dkept))
        L.check(rc, "mae_decoder_tokens_cls_bwd")

    def enc_chain(s):           # the masking gather of the parent's plan path, then fastvim_mae.py's cat chain
        kept = MT.gather_tokens(s["full"], plan.keep_index, plan.restore_index)
        M = kept.shape[1]
        cls_tokens = (vec + pos[:, :1, :]).expand(B, -1, -1).to(kept.dtype)
        return torch.cat((kept[:, :M // 2, :], cls_tokens, kept[:, M // 2:, :]), dim=1)

    def enc_bwd_chain(s):       # what autograd runs behind enc_chain, as plain ops: the cat's two slices, the gather's adjoint, the sum
        d, c = s["dkept1"], K // 2
        dk = torch.cat((d[:, :c, :], d[:, c + 1:, :]), dim=1)
        return MT._gather(dk, plan.restore_index, bf), d[:, c, :].float().sum(0)

    def dec_bwd_chain(s):       # the same behind dec_chain: casts, the gather's scatter-add, the repeat's sum, the slices
        d, c = s["dgrid1"], K // 2
        dcls, dgrid = d[:, Ln:, :].to(bf), d[:, :Ln, :].to(bf)
        g_ = torch.zeros(B, Ln, D, device=d.device, dtype=bf).scatter_add_(1, plan.ids_restore.unsqueeze(-1).expand(-1, -1, D), dgrid)
        dmask = g_[:, K:, :].float().sum((0, 1))
        return torch.cat([g_[:, :c, :], dcls, g_[:, c:K, :]], dim=1), dmask

    enc = lambda s: MT.encoder_tokens_cls(s["full"], vec, pos, plan)
    dec = lambda s: MT.decoder_tokens_cls(s["kept1"], vec, pos, plan)

    def dec_chain(s):           # fastvim_mae.py's forward_decoder between decoder_embed and the blocks
        x, c = s["kept1"], K // 2
        mask_tokens = vec.repeat(B, Ln - K, 1).to(x.dtype)
        x_ = torch.cat([x[:, :c, :], x[:, c + 1:, :], mask_tokens], dim=1)
        x_ = torch.gather(x_, dim=1, index=plan.ids_restore.unsqueeze(-1).repeat(1, 1, D))
        x_ = x_ + pos[:, 1:]
        cls_tokens = x[:, c:c + 1, :] + pos[:, :1, :]
        return torch.cat([x_, cls_tokens.to(x_.dtype)], dim=1)

    k1, full_b, grid1 = B * (K + 1) * D * 2, B * Ln * D * 2, B * (Ln + 1) * D * 4
    enc_f, enc_b = B * K * D * 2 + k1, k1 + full_b
    dec_f, dec_b = k1 + (Ln + 1) * D * 4 + grid1, grid1 + k1 + nblocks * D * 16
    rows = (
        ("encoder tokens fwd: launch", enc, ("full",), enc_f),
        ("encoder tokens fwd: torch chain", enc_chain, ("full",), enc_f),
        ("encoder tokens bwd: launch (2 kernels)", enc_bwd, ("dkept1",), enc_b),
        ("encoder tokens bwd: torch adjoint chain", enc_bwd_chain, ("dkept1",), enc_b),
        ("decoder tokens fwd: launch", dec, ("kept1",), dec_f),
        ("decoder tokens fwd: torch chain", dec_chain, ("kept1",), dec_f),
        ("decoder tokens bwd: launch (2 kernels)", dec_bwd, ("dgrid1",), dec_b),
        ("decoder tokens bwd: torch adjoint chain", dec_bwd_chain, ("dgrid1",), dec_b),
    )
    res = {}
    for rep in (1, 2):
        for name, fn, names, nbytes in rows:
            us = time_kernel(rotating(fn, T, names, nbytes)) * 1e6
            fl = floor_us(curve, nbytes / 1e6)
            rec = {"us": round(us, 2), "MB": round(nbytes / 1e6, 2), "floor_us": round(fl, 2), "floor_ratio": round(us / fl, 2),
                   "TBps": round(nbytes / us / 1e6, 3)}
            say(f"    [{rep}] {name:<40} {us:8.1f} us  {nbytes / 1e6:7.1f} MB  {rec['TBps']:.2f} TB/s  copy {fl:7.1f} us  "
                f"floor_ratio {rec['floor_ratio']:.2f}")
            res[f"{name} #{rep}"] = rec
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8, help="calls (micro-batches) per timed round, rounded to whole groups of 2")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--log", default=os.path.join(R, "profiles", "vim_mae_step_bench.log"))
    args = ap.parse_args()
    import torch
    import fastvim_amd  # noqa: F401  (sets the graph-capture switch before HIP initialises)
    if not torch.cuda.is_available():
        raise SystemExit("bench_vim_mae_step.py needs a GPU")
    lines, out = [], {}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush_log():
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")

    say(f"{torch.cuda.get_device_name()}: Vim MAE pre-training step object and class-token assembly")
    if not args.no_step:
        out["step"] = steps_part(args.batch, args.rounds, args.steps, say)
        torch.cuda.empty_cache()
        flush_log()
    if not args.no_kernels:
        from bench import floor_curve
        with phase("copy floor", 240, say):
            curve = floor_curve(torch.bfloat16, sizes_mb=(8, 16, 32, 64, 112, 160))
            say("  copy floor (MB moved, us): " + ", ".join(f"({a:.0f}, {b:.1f})" for a, b in curve))
            out["floor_curve"] = [(round(a, 1), round(b, 2)) for a, b in curve]
        out["kernels"] = {}
        for B, H, W, K, D in KERNEL_SHAPES:
            with phase(f"class-token launches at ({B}, {H * W} -> {K} + 1, {D}), bf16 tokens, HBM-cold", 420, say):
                out["kernels"][f"({B}, {H * W} -> {K} + 1, {D})"] = kernel_rows(B, H, W, K, D, curve, say)
            torch.cuda.empty_cache()
            flush_log()
    lines.append(json.dumps(out))
    print(lines[-1])
    flush_log()


if __name__ == "__main__":
    main()
