"""Time the device-side RandAugment (fastvim_amd/randaug.py, csrc/randaug.hip) and the host work it replaces, in ONE process,
for B = 128 images of 224 x 224 and the recipe ``rand-m9-mstd0.5-inc1`` (two layers):

  (a) HBM-cold (operand sets rotated past the Infinity Cache, bench.py's ``rotating``): the four launches -- statistics and
      apply of each layer -- for a DRAWN plan of the recipe (half of the layers skipped, the ops mixed within the batch) and
      for plans that force ONE op in both layers of every sample, next to a plain copy that moves the same number of bytes
      (each layer reads and writes the uint8 batch) in the same run, with the ratio of the two: the ``floor_ratio`` convention
      of bench.py's kernel rows.  Every row is timed twice, so the log shows the run's own spread;
  (b) the host: images per second of ONE core running the same drawn ops with PIL on 224 x 224 images (timm's op functions,
      tests/golden/gen_randaug.py), and the cores that 8 GPUs at bench.py's image rate would keep busy with that alone.

    python tools/bench_randaug.py            # --no-gpu: the host part only

Every GPU step runs under a time limit of its own (``--limit`` seconds, bench_u8's watchdog: exit code 124, nothing further
is started).  Reads nothing outside the repository and sets no threshold.  The log goes to stdout and to ``--log``
(profiles/randaug_bench.log), the last line one JSON record."""
import argparse
import importlib.util
import json
import os
import random
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import fastvim_amd  # noqa: E402,F401  (sets the graph-capture switch before HIP initialises)
from fastvim_amd.randaug import OPS_INCREASING, RandAugment  # noqa: E402

B, S = 128, 224
RECIPE = "rand-m9-mstd0.5-inc1"
MEAN = (0.485, 0.456, 0.406)
STEP_IMG_PER_S = 24500.0      # bench.py's FastVim-T rate per GPU that the recipe stands for (README)


def forced_plan(ra, name, seed):
    """op ``name`` in both layers of every sample, its argument drawn as the recipe draws it"""
    random.seed(seed)
    for k in range(ra.batch):
        for layer in range(ra.num_layers):
            m = max(0., min(random.gauss(ra.magnitude, ra.magnitude_std), ra.upper_bound))
            ra.put(k, layer, ra.record(name, *ra.level_args(name, m)))


def drawn_plan(ra, seed):
    np.random.seed(seed)
    random.seed(seed)
    return [ra.draw(k) for k in range(ra.batch)]


def gpu_part(say, rec, limit):
    from bench import rotating, time_kernel
    from bench_u8 import limited
    from fastvim_amd import _lib as L
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    lib = L.lib()
    nb = B * 3 * S * S
    ra = RandAugment(RECIPE, S, MEAN, B)
    ra.commit()                                    # allocates the device plan and the workspace
    x = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8, device="cuda")
    base = {"src": x, "tmp": torch.empty_like(x), "out": torch.empty_like(x)}
    b, s, nl = L.i32(B), L.i32(S), L.i32(ra.num_layers)
    plan, ws = L.ptr(ra._plan_dev), L.ptr(ra._ws)

    def four(st_):
        st = L.stream_of(st_["out"])
        for layer, (src, dst) in enumerate(((st_["src"], st_["tmp"]), (st_["tmp"], st_["out"]))):
            L.check(lib.fv_randaug_stats(L.ptr(src), plan, ws, b, s, s, nl, L.i32(layer), st), "fv_randaug_stats")
            L.check(lib.fv_randaug_apply(L.ptr(src), L.ptr(dst), plan, ws, b, s, s, nl, L.i32(layer), st), "fv_randaug_apply")

    nbytes = 4 * nb                                # two layers, each reads and writes the batch
    cbase = {"a": torch.randint(0, 256, (2 * nb,), dtype=torch.uint8, device="cuda"),
             "b": torch.empty(2 * nb, dtype=torch.uint8, device="cuda")}

    def cold(fn, bs, names):
        fns = rotating(fn, bs, names, nbytes, cap=16)
        us = time_kernel(fns) * 1e6
        del fns
        return us

    say(f"(a) HBM-cold, B = {B} at {S} x {S}, two layers = four launches (us, each row timed twice; {nbytes / 1e6:.1f} MB = each "
        f"layer reads and writes the {nb / 1e6:.2f} MB batch; the copy row moves the same total in one launch):")
    with limited(limit, "plain copy"):
        tc = [cold(lambda st_: st_["b"].copy_(st_["a"]), cbase, ("a", "b")) for _ in range(2)]
    say(f"    {'plain copy, same bytes':28s}: {tc[0]:8.2f} {tc[1]:8.2f} us   {nbytes / min(tc) / 1e6:.2f} TB/s")
    rows = {"plain copy, same bytes": [round(v, 2) for v in tc]}
    plans = [("drawn plan of the recipe", None)] + [(n, n) for n in OPS_INCREASING]
    for label, name in plans:
        if name is None:
            drawn = drawn_plan(ra, 1)
            skipped = sum(n is None for layers in drawn for n, _ in layers)
            label = f"drawn plan ({skipped} of {2 * B} layers skipped)"
        else:
            forced_plan(ra, name, 2)
        ra.commit()
        torch.cuda.synchronize()
        with limited(limit, label):
            t = [cold(four, base, ("src", "tmp", "out")) for _ in range(2)]
        rows[label] = [round(v, 2) for v in t]
        say(f"    {label:28s}: {t[0]:8.2f} {t[1]:8.2f} us   floor_ratio {min(t) / min(tc):5.2f}")
        if name is None:
            rec["drawn_us"], rec["drawn_floor_ratio"] = round(min(t), 2), round(min(t) / min(tc), 2)
            say(f"      = {min(t) / 5000 * 100:.1f} % of a 5 ms FastVim-T step")
    rec["rows_us"] = rows


def host_part(say, rec, n_images):
    try:
        from PIL import Image
    except ImportError:
        say("(b) host: PIL is not importable here; not measured")
        return
    spec = importlib.util.spec_from_file_location("gen_randaug", os.path.join(R, "tests", "golden", "gen_randaug.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    import PIL
    ra = RandAugment(RECIPE, S, MEAN, 1)
    rng = np.random.default_rng(0)
    # random contents: the cost of PIL's point / blend / filter / transform does not depend on them
    imgs = [Image.fromarray(rng.integers(0, 256, (S, S, 3), dtype=np.uint8)) for _ in range(16)]
    np.random.seed(3)
    random.seed(3)
    plans = [ra.draw(0) for _ in range(n_images)]
    torch.set_num_threads(1)
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        for i, layers in enumerate(plans):
            img = imgs[i % 16]
            for name, args in layers:
                if name is not None:
                    img = gen.pil_op(name, img, args, ra.fill)
        times.append(time.perf_counter() - t0)
    per_core = n_images / min(times)
    cores = 8 * STEP_IMG_PER_S / per_core
    say(f"(b) host, PIL {PIL.__version__}, one core, the recipe's drawn ops on {S} x {S} images ({n_images} images, best of 3 passes: "
        f"{[round(t, 3) for t in times]} s):")
    say(f"    {per_core:8.0f} images/s per core; 8 GPUs at {STEP_IMG_PER_S:.0f} images/s each would keep {cores:.0f} cores busy with "
        "RandAugment alone (decode, crop and collate not counted)")
    rec["host_img_per_s_per_core"], rec["host_cores_for_8_gpus"] = round(per_core), round(cores, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--limit", type=float, default=120.0, help="seconds each GPU step may take")
    ap.add_argument("--no-gpu", action="store_true", help="the host part only")
    ap.add_argument("--host-images", type=int, default=2000)
    ap.add_argument("--log", default=os.path.join(R, "profiles", "randaug_bench.log"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rec = {"batch": B, "size": S, "config": RECIPE}
    if not a.no_gpu:
        assert torch.cuda.is_available(), "bench_randaug.py needs a GPU (or --no-gpu)"
        gpu_part(say, rec, a.limit)
    host_part(say, rec, a.host_images)
    say(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    with open(a.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
