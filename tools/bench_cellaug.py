"""Time the device-side cell augmentation (fastvim_amd/cellaug.py, csrc/cellaug.hip) on the GPU, in ONE process, for
B = 64 cell images of 8 channels augmented to 224 x 224 from sources with sides 96 .. 288:

  (a) HBM-cold (operand sets rotated past the Infinity Cache, bench.py's ``rotating``): each launch and the pair, for a DRAWN
      batch of the recipe (every step fires with probability 0.5) and with EVERY op forced on (rotation, radius-3 defocus, 10
      holes in every sample), each next to a plain copy that moves the same number of bytes, with the ratio of the two (the
      ``floor_ratio`` convention of bench.py's kernel rows).  Every row is timed twice, so the log shows the run's own spread;
  (b) the pinned host-to-device copy of the staged planes next to the copy of the fp32 batch it replaces;
  (c) the host's share per sample: ``draw`` + ``put`` (plan, record and the copy into the pool).

The host side of the comparison -- the recipe as albumentations / OpenCV run it per sample -- is NOT measured: neither is a
dependency of this project.

    python tools/bench_cellaug.py

Every GPU step runs under a time limit of its own (``--limit`` seconds, bench_u8's watchdog: exit code 124, nothing further
is started).  Reads nothing outside the repository and sets no threshold.  The log goes to stdout and to ``--log``
(profiles/cellaug_bench.log), the last line one JSON record."""
import argparse
import json
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import fastvim_amd  # noqa: E402,F401  (sets the graph-capture switch before HIP initialises)
from bench import rotating, time_kernel  # noqa: E402
from bench_u8 import limited  # noqa: E402
from fastvim_amd import cellaug as CA  # noqa: E402

B, C, S = 64, 8, 224


def staged(kind, seed):
    """The host half of one batch (plain numpy): plan table, the pool trimmed to the bytes in use, and what fired."""
    rng = np.random.default_rng(seed)
    aug = CA.CellAugmentation(S, seed=seed)
    hp = CA.HostCellPlan(B, C, S, capacity_bytes=B * (C * 288 * 288 + 16))
    fired = {"flip": 0, "rotate": 0, "defocus": 0, "dropout": 0}
    imgs = [rng.integers(0, 256, (C, int(rng.integers(96, 289)), int(rng.integers(96, 289))), dtype=np.uint8) for _ in range(B)]
    t0 = time.perf_counter()
    for k, img in enumerate(imgs):
        p = aug.draw(img.shape[1], img.shape[2])
        if kind == "forced":
            holes = p.holes or tuple((11 * j, 17 * j, 11 * j + 10, 17 * j + 10) for j in range(10))
            p = CA.CellPlan(p.oy, p.ox, CA.ROTATE, p.angle if p.op == CA.ROTATE else 33.0 + k, 3, p.sigma or 0.3, holes)
        fired["flip"] += p.op in (CA.HFLIP, CA.VFLIP)
        fired["rotate"] += p.op == CA.ROTATE
        fired["defocus"] += p.radius > 0
        fired["dropout"] += len(p.holes) > 0
        hp.put(k, img, p)
    host_us = (time.perf_counter() - t0) / B * 1e6
    hp.check_complete()
    used = (hp.used + 15) // 16 * 16
    return hp.plan.copy(), hp.pool[:used].copy(), hp.used, fired, host_us


def cold(fn, base, names, nbytes):
    fns = rotating(fn, base, names, nbytes, cap=16)
    us = time_kernel(fns) * 1e6
    del fns
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--limit", type=float, default=120.0, help="seconds each GPU step may take")
    ap.add_argument("--log", default=os.path.join(R, "profiles", "cellaug_bench.log"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    assert torch.cuda.is_available(), "bench_cellaug.py needs a GPU"
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    out_bytes = B * C * S * S
    rec = {"batch": B, "channels": C, "size": S, "out_MB": round(out_bytes / 1e6, 2)}
    say(f"(a) HBM-cold, B = {B}, C = {C} to {S} x {S}, sources with sides 96 .. 288 (us per launch, each row timed twice; the copy "
        "row under a row moves the same bytes):")
    for kind in ("drawn", "forced"):
        plan, pool, used, fired, host_us = staged(kind, seed=1)
        d_plan = torch.from_numpy(plan).cuda()
        base = {"pool": torch.from_numpy(pool).cuda(),
                "mid": torch.randint(0, 256, (B, C, S, S), dtype=torch.uint8, device="cuda"),
                "out": torch.empty(B, C, S, S, dtype=torch.uint8, device="cuda")}

        def geom(st_):
            CA.geom(st_["pool"], d_plan, st_["mid"])

        def filt(st_):
            CA.filter(st_["mid"], d_plan, st_["out"])

        def pair(st_):
            geom(st_)
            filt(st_)

        say(f"  {kind}: {used / 1e6:.1f} MB staged; of {B} samples {fired['flip']} flip, {fired['rotate']} rotate, "
            f"{fired['defocus']} defocus, {fired['dropout']} drop holes")
        r = {"staged_MB": round(used / 1e6, 2), "fired": {k: int(v) for k, v in fired.items()}}
        rows = [("geometry", geom, ("pool", "mid"), used + out_bytes), ("defocus + holes", filt, ("mid", "out"), 2 * out_bytes),
                ("both launches", pair, ("pool", "mid", "out"), used + 3 * out_bytes)]
        for name, fn, names, nbytes in rows:
            half = nbytes // 2
            cbase = {"a": torch.randint(0, 256, (half,), dtype=torch.uint8, device="cuda"),
                     "b": torch.empty(half, dtype=torch.uint8, device="cuda")}
            with limited(a.limit, f"{kind} {name}"):
                t = [cold(fn, base, names, nbytes) for _ in range(2)]
            with limited(a.limit, f"{kind} {name} copy"):
                tc = [cold(lambda st_: st_["b"].copy_(st_["a"]), cbase, ("a", "b"), nbytes) for _ in range(2)]
            del cbase
            ratio = min(t) / min(tc)
            r[name] = {"us": [round(v, 2) for v in t], "copy_us": [round(v, 2) for v in tc], "MB": round(nbytes / 1e6, 1),
                       "floor_ratio": round(ratio, 2)}
            say(f"    {name:16s}: {t[0]:8.2f} {t[1]:8.2f} us   {nbytes / 1e6:6.1f} MB   {nbytes / min(t) / 1e6:.2f} TB/s   "
                f"copy of the same bytes {tc[0]:7.2f} {tc[1]:7.2f} us   floor_ratio {ratio:.2f}")
        rec[kind] = r
        if kind == "drawn":
            rec["host_us_per_sample"] = round(host_us, 1)
            # (b) the link: the staged planes against the fp32 batch a host-side recipe sends
            pin_pool = torch.from_numpy(pool).pin_memory()
            pin_x = torch.empty(B, C, S, S, dtype=torch.float32).pin_memory()
            d_x = torch.empty(B, C, S, S, dtype=torch.float32, device="cuda")
            link = {}
            for name, dst, src in (("staged planes", base["pool"], pin_pool), ("fp32 batch", d_x, pin_x)):
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
                nb = src.numel() * src.element_size()
                link[name] = {"MB": round(nb / 1e6, 2), "us": [round(ts[0], 1), round(ts[len(ts) // 2], 1), round(ts[-1], 1)]}
            say("(b) pinned host-to-device copy, us [min, median, max] of 5 after 2 warm-up copies:")
            for name, v in link.items():
                say(f"    {name:14s}: {v['MB']:7.2f} MB   {v['us']}   {v['MB'] / v['us'][1] * 1e3:.1f} GB/s")
            link["bytes_ratio"] = round(link["staged planes"]["MB"] / link["fp32 batch"]["MB"], 2)
            say(f"    staged bytes / fp32 batch bytes: {link['bytes_ratio']:.2f}")
            rec["link"] = link
            say(f"(c) host: draw + put (plan, record, copy into the pool) {host_us:.1f} us per sample, one thread, pageable pool; "
                "the recipe on the host (albumentations / OpenCV) is not measured -- neither is a dependency")
            del pin_pool, pin_x, d_x
        del base
        torch.cuda.empty_cache()
    say(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    with open(a.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
