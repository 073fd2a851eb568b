"""Time the device-side geometry (fastvim_amd/resample.py, csrc/resample.hip) on the GPU, in ONE process, for B = 128 images
resampled to 224 x 224 from sources drawn like ImageNet (sides 200 .. 600):

  (a) HBM-cold (operand sets rotated past the Infinity Cache, bench.py's ``rotating``): the two launches -- coefficients, then
      pixels -- for the training plan (random resized crop at scale 0.2 .. 1, half the samples flipped) and for the
      validation plan (whole image, short side to 256, centre 224), each next to a plain copy that moves the same number of
      bytes (the staged source bytes read + the uint8 batch written), with the ratio of the two: the ``floor_ratio``
      convention of bench.py's kernel rows.  Every row is timed twice, so the log shows the run's own spread;
  (b) the pinned host-to-device copy of the staged crops next to the copy of the 19 MB uint8 batch it replaces, and the
      ratio of the bytes: the link carries MORE with the geometry on the device, because the crops are larger than 224 x 224.

    python tools/bench_resample.py

Every GPU step runs under a time limit of its own (``--limit`` seconds, bench_u8's watchdog: exit code 124, nothing further
is started).  Reads nothing outside the repository and sets no threshold.  The log goes to stdout and to ``--log``
(profiles/resample_bench.log), the last line one JSON record."""
import argparse
import ctypes
import json
import os
import random
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import fastvim_amd  # noqa: E402,F401  (sets the graph-capture switch before HIP initialises)
from bench import rotating, time_kernel  # noqa: E402
from bench_u8 import limited  # noqa: E402
from fastvim_amd import _lib as L  # noqa: E402
from fastvim_amd.resample import HostPlan, RandomResizedCrop, ResizeCenterCrop, workspace_ints  # noqa: E402

B, S = 128, 224


def sources(rng):
    """(H, W) of B decoded images, sides 200 .. 600 (ImageNet's are mostly 500 x 375 and around it); contents random."""
    return [(rng.randint(200, 600), rng.randint(200, 600)) for _ in range(B)]


def staged(kind, sizes, seed):
    """The host half of one batch: plan and pool (plain numpy), the pool trimmed to the bytes in use."""
    nprng = np.random.default_rng(seed)
    random.seed(seed)
    rrc = RandomResizedCrop(S, scale=(0.2, 1.0), generator=torch.Generator().manual_seed(seed))
    rcc = ResizeCenterCrop(S)
    hp = HostPlan(B, S, capacity_bytes=B * 600 * 600 * 3 + 16 * B)
    area = 0.0
    for k, (H, W) in enumerate(sizes):
        img = nprng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        if kind == "train":
            i, j, h, w, f = rrc.draw(H, W)
            hp.put(k, img, crop=(i, j, h, w), flip=f)
            area += h * w / (H * W)
        else:
            out_full, window = rcc.plan(H, W)
            hp.put(k, img, out_full=out_full, window=window)
            area += 1.0
    hp.check_complete()
    used = (hp.used + 15) // 16 * 16
    return hp.plan.copy(), hp.pool[:used].copy(), hp.used, area / B, hp.fallbacks


def cold(fn, base, names, nbytes):
    fns = rotating(fn, base, names, nbytes, cap=16)
    us = time_kernel(fns) * 1e6
    del fns
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--limit", type=float, default=120.0, help="seconds each GPU step may take")
    ap.add_argument("--log", default=os.path.join(R, "profiles", "resample_bench.log"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    assert torch.cuda.is_available(), "bench_resample.py needs a GPU"
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    lib = L.lib()
    sizes = sources(random.Random(0))
    out_bytes = B * 3 * S * S
    rec = {"batch": B, "size": S, "out_MB": round(out_bytes / 1e6, 2)}
    ws = torch.empty(workspace_ints(B, S, S), dtype=torch.int32, device="cuda")
    b, s = L.i32(B), L.i32(S)
    say(f"(a) HBM-cold, B = {B} to {S} x {S}, sources with sides 200 .. 600 (us per launch, each row timed twice; MB = source "
        f"bytes staged + {out_bytes / 1e6:.2f} MB written; the copy row moves the same total):")
    for kind in ("train", "val"):
        plan, pool, used, area, fallbacks = staged(kind, sizes, seed=1)
        d_plan = torch.from_numpy(plan).cuda()
        base = {"pool": torch.from_numpy(pool).cuda(), "out": torch.empty(B, 3, S, S, dtype=torch.uint8, device="cuda")}
        nb = ctypes.c_longlong(base["pool"].numel())
        nbytes = used + out_bytes

        def coeffs(st_):
            L.check(lib.fv_resample_coeffs(L.ptr(d_plan), nb, L.ptr(ws), b, s, s, L.stream_of(st_["out"])), "fv_resample_coeffs")

        def pixels(st_):
            L.check(lib.fv_resample_u8(L.ptr(st_["pool"]), nb, L.ptr(d_plan), L.ptr(ws), L.ptr(st_["out"]), b, s, s,
                                       L.stream_of(st_["out"])), "fv_resample_u8")

        def both(st_):
            coeffs(st_)
            pixels(st_)

        half = nbytes // 2
        cbase = {"a": torch.randint(0, 256, (half,), dtype=torch.uint8, device="cuda"),
                 "b": torch.empty(half, dtype=torch.uint8, device="cuda")}
        rows = [("coefficients", coeffs, base, ("pool", "out")), ("pixels", pixels, base, ("pool", "out")),
                ("both launches", both, base, ("pool", "out")), ("plain copy, same bytes", lambda st_: st_["b"].copy_(st_["a"]), cbase, ("a", "b"))]
        say(f"  {kind}: source area staged = {area:.2f} of the image on average, {used / 1e6:.1f} MB staged, {fallbacks} host fallbacks")
        r = {"staged_MB": round(used / 1e6, 2), "area_fraction": round(area, 3), "fallbacks": fallbacks}
        for name, fn, bs, names in rows:
            with limited(a.limit, f"{kind} {name}"):
                t = [cold(fn, bs, names, nbytes) for _ in range(2)]
            r[name] = [round(v, 2) for v in t]
            say(f"    {name:24s}: {t[0]:8.2f} {t[1]:8.2f} us   {nbytes / 1e6:6.1f} MB   {nbytes / min(t) / 1e6:.2f} TB/s")
        ratio = min(r["both launches"]) / min(r["plain copy, same bytes"])
        r["floor_ratio"] = round(ratio, 2)
        say(f"    both launches / copy of the same bytes (floor_ratio): {ratio:.2f}")
        rec[kind] = r
        if kind == "train":
            # (b) the link: the staged crops against the finished uint8 batch
            pin_pool = torch.from_numpy(pool).pin_memory()
            pin_x = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8).pin_memory()
            d_x = torch.empty_like(pin_x, device="cuda")
            link = {}
            for name, dst, src in (("staged crops", base["pool"], pin_pool), ("uint8 batch", d_x, pin_x)):
                with limited(a.limit, f"h2d {name}"):
                    ts = []
                    for _ in range(7):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        dst.copy_(src, non_blocking=True)
                        e1.record()
                        e1.synchronize()
                        ts.append(e0.elapsed_time(e1) * 1e3)
                    ts = sorted(ts[2:])
                link[name] = {"MB": round(src.numel() / 1e6, 2), "us": [round(ts[0], 1), round(ts[len(ts) // 2], 1), round(ts[-1], 1)]}
            say("(b) pinned host-to-device copy, us [min, median, max] of 5 after 2 warm-up copies:")
            for name, v in link.items():
                say(f"    {name:14s}: {v['MB']:6.2f} MB   {v['us']}   {v['MB'] / v['us'][1] * 1e3:.1f} GB/s")
            link["bytes_ratio"] = round(link["staged crops"]["MB"] / link["uint8 batch"]["MB"], 2)
            say(f"    staged bytes / uint8 batch bytes: {link['bytes_ratio']:.2f} (the link carries more with the geometry on the device)")
            rec["link"] = link
        del base, cbase
        torch.cuda.empty_cache()
    say(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    with open(a.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
