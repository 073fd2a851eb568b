"""Time the JPEG path (fastvim_amd/jpeg.py, csrc/jpeg_host.cpp, csrc/jpeg.hip) in ONE process, for B = 128 synthetic
photograph-like JPEG files PIL encodes here (sides 200 .. 600, quality 75 .. 95, half 4:2:0 and half 4:4:4; smooth
low-frequency content plus grain) and crops drawn by ``RandomResizedCrop(224)``:

  (a) HOST time per image of ``put_jpeg`` (probe + entropy decoding of the crop's MCU window into the pinned pool) against
      ``Image.open(...).convert("RGB")`` + ``put`` on the same files with the same crops, on one thread and on several; the
      entropy decoder alone on whole images, for the share of a full decode it is;
  (b) HBM-cold (operand sets rotated past the Infinity Cache, bench.py's ``rotating``) the two launches next to a plain copy
      that moves the same number of bytes (coefficients read, planes written and read, crops written), with the ratio of
      the two: the ``floor_ratio`` convention of bench.py's kernel rows.  Every row is timed twice;
  (c) the link: coefficient bytes staged against the RGB crop bytes ``put`` would have staged;
  (d) the PACKED coefficient form (``coef_format="packed"``) next to the dense one, same process, files and crops: bytes
      staged per batch against the dense form and the RGB crops; host time per image of ``put_jpeg``, dense and packed
      passes alternating; the pinned copy of each; ``fv_jpeg_idct_packed`` against ``fv_jpeg_idct`` HBM-cold, each twice
      and each next to a plain copy of its own bytes.  The planes of the two are compared byte for byte first.  These
      rows also go to ``--packed-log`` (profiles/jpeg_packed_bench.log).

    python tools/bench_jpeg.py

Every GPU step runs under a time limit of its own (``--limit`` seconds, bench_u8's watchdog).  Reads nothing outside the
repository and sets no threshold.  The log goes to stdout and to ``--log`` (profiles/jpeg_bench.log), the last line one
JSON record."""
import argparse
import ctypes
import io
import json
import os
import random
import sys
import time
from concurrent.futures import ThreadPoolExecutor

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import fastvim_amd  # noqa: E402,F401  (sets the graph-capture switch before HIP initialises)
from bench import rotating, time_kernel  # noqa: E402
from bench_u8 import limited  # noqa: E402
from fastvim_amd import _lib as L  # noqa: E402
from fastvim_amd import jpeg  # noqa: E402
from fastvim_amd.resample import RandomResizedCrop  # noqa: E402

B, S = 128, 224


def files(seed):
    """B JPEG files: a smooth field (a 12 x 12 random image enlarged bicubically) plus grain of sigma 5."""
    from PIL import Image
    rng, out = np.random.default_rng(seed), []
    for k in range(B):
        H, W = int(rng.integers(200, 601)), int(rng.integers(200, 601))
        low = Image.fromarray(rng.integers(0, 256, (12, 12, 3), dtype=np.uint8)).resize((W, H), Image.BICUBIC)
        a = np.clip(np.asarray(low).astype(np.float32) + rng.normal(0, 5, (H, W, 3)), 0, 255).astype(np.uint8)
        b = io.BytesIO()
        Image.fromarray(a).save(b, "JPEG", quality=int(rng.integers(75, 96)), subsampling=(2, 0)[k & 1])
        out.append(b.getvalue())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--limit", type=float, default=120.0, help="seconds each GPU step may take")
    ap.add_argument("--threads", type=int, default=8, help="loader threads of the multi-thread rows")
    ap.add_argument("--log", default=os.path.join(R, "profiles", "jpeg_bench.log"))
    ap.add_argument("--packed-log", default=os.path.join(R, "profiles", "jpeg_packed_bench.log"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    from PIL import Image, features
    import PIL
    assert torch.cuda.is_available(), "bench_jpeg.py needs a GPU"
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; PIL {PIL.__version__}, libjpeg-turbo "
        f"{features.version('jpg')}")
    raws = files(0)
    infos = [jpeg.probe(r) for r in raws]
    assert all(i.served for i in infos)
    random.seed(1)
    rrc = RandomResizedCrop(S, generator=torch.Generator().manual_seed(1))
    draws = [rrc.draw(i.height, i.width) for i in infos]
    px = sum(i.height * i.width for i in infos)
    say(f"{B} files, {sum(map(len, raws)) / B / 1e3:.1f} KB and {px / B / 1e3:.0f} kilopixels on average; crops cover "
        f"{sum(d[2] * d[3] for d in draws) / px:.2f} of the pixels")
    stage = jpeg.JpegImageStage(B, S, capacity_bytes=B * 600 * 600 * 3 + 16 * B, coef_capacity_bytes=B * 608 * 608 * 6, slots=1)
    rec = {"batch": B, "size": S, "file_KB": round(sum(map(len, raws)) / B / 1e3, 1)}

    # ------------------------------------------------------------------------------------------------------ (a) host
    def put_file(k):
        i, j, h, w, f = draws[k]
        stage.put_jpeg(k, raws[k], crop=(i, j, h, w), flip=f)

    def put_pil(k):
        i, j, h, w, f = draws[k]
        stage.put(k, np.asarray(Image.open(io.BytesIO(raws[k])).convert("RGB")), crop=(i, j, h, w), flip=f)

    def pil_only(k):
        np.asarray(Image.open(io.BytesIO(raws[k])).convert("RGB"))

    def entropy_whole(k):
        jpeg.entropy_decode(raws[k])

    def host_row(name, fn, threads, commit):
        ts = []
        for _ in range(4):
            t0 = time.perf_counter()
            if threads == 1:
                for k in range(B):
                    fn(k)
            else:
                with ThreadPoolExecutor(threads) as ex:
                    list(ex.map(fn, range(B)))
            ts.append((time.perf_counter() - t0) / B * 1e3)
            if commit:
                stage.commit()
                torch.cuda.synchronize()
        ts = ts[1:]                                        # the first pass warms caches and allocators
        say(f"    {name:46s} {threads:2d} thread(s): {min(ts):7.3f} ms per image (wall / {B}; passes: {', '.join(f'{t:.3f}' for t in ts)})")
        return round(min(ts), 4)

    say("(a) host time per image, the same files and crops, one process (the minimum of three passes after a warm-up pass):")
    host = {}
    with limited(4 * a.limit, "host rows"):
        for threads in (1, a.threads):
            host[f"put_jpeg_{threads}"] = host_row("put_jpeg (probe + entropy decode of the window)", put_file, threads, True)
            fallbacks = stage.last_jpeg_fallbacks
            host[f"pil_put_{threads}"] = host_row("Image.open().convert('RGB') + put", put_pil, threads, True)
            host[f"pil_decode_{threads}"] = host_row("Image.open().convert('RGB') alone", pil_only, threads, False)
            host[f"entropy_whole_{threads}"] = host_row("entropy decode alone, WHOLE image", entropy_whole, threads, False)
    host["ratio_1"] = round(host["put_jpeg_1"] / host["pil_put_1"], 3)
    host[f"ratio_{a.threads}"] = round(host[f"put_jpeg_{a.threads}"] / host[f"pil_put_{a.threads}"], 3)
    say(f"    put_jpeg / (PIL decode + put): {host['ratio_1']:.2f} on one thread, {host[f'ratio_{a.threads}']:.2f} on {a.threads}; "
        f"{fallbacks} fallbacks")
    rec["host_ms_per_image"] = host

    # ---------------------------------------------------------------------------------------------------- (b) device
    for k in range(B):
        put_file(k)
    stage.commit()
    torch.cuda.synchronize()
    s = stage._ready
    elems, crop_bytes = s.jused, stage.staged_bytes
    table = s.table
    base = {"coef": s.coef[:elems].clone(), "planes": torch.empty(elems, dtype=torch.uint8, device="cuda"),
            "pool": torch.empty((crop_bytes + 15) // 16 * 16 + 16 * B, dtype=torch.uint8, device="cuda")}
    ne, nb, b = ctypes.c_longlong(elems), ctypes.c_longlong(base["pool"].numel()), L.i32(B)
    lib = L.lib()

    def idct(st_):
        L.check(lib.fv_jpeg_idct(L.ptr(st_["coef"]), ne, L.ptr(table), L.ptr(st_["planes"]), ne, b, L.stream_of(st_["pool"])), "fv_jpeg_idct")

    def rgb(st_):
        L.check(lib.fv_jpeg_rgb(L.ptr(st_["planes"]), ne, L.ptr(table), L.ptr(st_["pool"]), nb, b, L.stream_of(st_["pool"])), "fv_jpeg_rgb")

    def both(st_):
        idct(st_)
        rgb(st_)

    nbytes = 2 * elems + elems + elems + crop_bytes
    half = nbytes // 2
    cbase = {"a": torch.randint(0, 256, (half,), dtype=torch.uint8, device="cuda"), "b": torch.empty(half, dtype=torch.uint8, device="cuda")}
    say(f"(b) HBM-cold, B = {B} (us per launch, each row timed twice; MB = {2 * elems / 1e6:.1f} coefficients read + {elems / 1e6:.1f} "
        f"planes written + read again + {crop_bytes / 1e6:.1f} crops written; the copy row moves the same total):")
    dev = {}
    rows = [("fv_jpeg_idct", idct, base, ("coef", "planes", "pool")), ("fv_jpeg_rgb", rgb, base, ("coef", "planes", "pool")),
            ("both launches", both, base, ("coef", "planes", "pool")),
            ("plain copy, same bytes", lambda st_: st_["b"].copy_(st_["a"]), cbase, ("a", "b"))]
    both(base)                                             # planes are written before fv_jpeg_rgb is timed alone
    torch.cuda.synchronize()
    for name, fn, bs, names in rows:
        with limited(a.limit, name):
            fns = rotating(fn, bs, names, nbytes, cap=16)      # clones: every set has coefficients and planes of its own
            t = []
            for _ in range(2):
                t.append(time_kernel(fns) * 1e6)
            del fns
        dev[name] = [round(v, 2) for v in t]
        say(f"    {name:24s}: {t[0]:8.2f} {t[1]:8.2f} us   {nbytes / 1e6:6.1f} MB   {nbytes / min(t) / 1e6:.2f} TB/s")
    dev["floor_ratio"] = round(min(dev["both launches"]) / min(dev["plain copy, same bytes"]), 2)
    say(f"    both launches / copy of the same bytes (floor_ratio): {dev['floor_ratio']:.2f}")
    say(f"    per image: {min(dev['both launches']) / B:.2f} us of device time")
    rec["device_us"] = dev

    # ------------------------------------------------------------------------------------------------------ (c) link
    rec["link"] = {"coef_MB": round(2 * elems / 1e6, 2), "crop_MB": round(crop_bytes / 1e6, 2), "bytes_ratio": round(2 * elems / crop_bytes, 2)}
    say(f"(c) link: {2 * elems / 1e6:.1f} MB of coefficients staged ({stage.staged_pool_bytes} pool bytes: the device fills the crops' "
        f"regions itself) against {crop_bytes / 1e6:.1f} MB of RGB crops from put: {2 * elems / crop_bytes:.2f}x the bytes")
    # ---------------------------------------------------------------------------------------------------- (d) packed
    mark = len(lines)
    del cbase, rows
    pstage = jpeg.JpegImageStage(B, S, capacity_bytes=B * 600 * 600 * 3 + 16 * B, coef_capacity_bytes=B * 608 * 608, slots=1,
                                 coef_format="packed", plane_capacity_bytes=B * 608 * 608 * 3)

    def put_packed(k):
        i, j, h, w, f = draws[k]
        pstage.put_jpeg(k, raws[k], crop=(i, j, h, w), flip=f)

    def put_row(name, st, fn, threads):
        t0 = time.perf_counter()
        if threads == 1:
            for k in range(B):
                fn(k)
        else:
            with ThreadPoolExecutor(threads) as ex:
                list(ex.map(fn, range(B)))
        t = (time.perf_counter() - t0) / B * 1e3
        st.commit()
        torch.cuda.synchronize()
        return t

    say("(d) the packed coefficient form next to the dense one")
    say("    host time per image of put_jpeg (the minimum of three passes after a warm-up pass; dense and packed passes alternate):")
    packed = {}
    with limited(4 * a.limit, "packed host rows"):
        for threads in (1, a.threads):
            td, tp = [], []
            for _ in range(4):
                td.append(put_row("dense", stage, put_file, threads))
                tp.append(put_row("packed", pstage, put_packed, threads))
            for name, ts in (("dense", td[1:]), ("packed", tp[1:])):
                packed[f"put_jpeg_{name}_{threads}"] = round(min(ts), 4)
                say(f"        put_jpeg, {name:6s} {threads:2d} thread(s): {min(ts):7.3f} ms per image (passes: {', '.join(f'{t:.3f}' for t in ts)})")
            say(f"        packed / dense on {threads} thread(s): {min(tp[1:]) / min(td[1:]):.2f}")
    # the batch both stages hold now was put on a.threads threads; put it once more in order, so that the plane layouts agree
    for k in range(B):
        put_file(k)
        put_packed(k)
    stage.commit()
    pstage.commit()
    torch.cuda.synchronize()
    assert pstage.last_jpeg_fallbacks == 0 and stage.last_jpeg_fallbacks == 0
    sp = pstage._ready
    pbytes = pstage.staged_coef_bytes
    blocks = int(sp.table_np[B * jpeg.REC_INTS + B])
    assert 64 * blocks == elems == sp.pused
    packed["bytes"] = {"packed_MB": round(pbytes / 1e6, 2), "dense_MB": round(2 * elems / 1e6, 2), "crop_MB": round(crop_bytes / 1e6, 2),
                       "dense_over_packed": round(2 * elems / pbytes, 2), "packed_over_crop": round(pbytes / crop_bytes, 2),
                       "bytes_per_block": round(pbytes / blocks, 1)}
    say(f"    bytes staged per batch: packed {pbytes / 1e6:.2f} MB ({pbytes / blocks:.1f} per block of {blocks}), dense {2 * elems / 1e6:.2f} MB "
        f"(128 per block): dense / packed = {2 * elems / pbytes:.2f}; RGB crops {crop_bytes / 1e6:.2f} MB: packed / crops = "
        f"{pbytes / crop_bytes:.2f} (dense / crops = {2 * elems / crop_bytes:.2f})")

    def link_row(name, dst, src):
        ts = []
        for _ in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src, non_blocking=True)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        nb_ = src.numel() * src.element_size()
        say(f"        {name:6s}: {min(ts[1:]):8.1f} us for {nb_ / 1e6:6.2f} MB ({nb_ / min(ts[1:]) / 1e3:.1f} GB/s; passes: "
            f"{', '.join(f'{t:.1f}' for t in ts[1:])})")
        return round(min(ts[1:]), 1)

    say("    the pinned copy of the coefficients, host to device (us, the minimum of five after a warm-up):")
    with limited(a.limit, "pinned copies"):
        packed["copy_us_dense"] = link_row("dense", s.coef[:elems], s.coef_pin[:elems])
        packed["copy_us_packed"] = link_row("packed", sp.coef[:pbytes], sp.coef_pin[:pbytes])
    say(f"        packed / dense: {packed['copy_us_packed'] / packed['copy_us_dense']:.2f}")

    dbase = {"coef": s.coef[:elems].clone(), "planes": torch.zeros(elems, dtype=torch.uint8, device="cuda")}
    pbase = {"coef": sp.coef[:pbytes].clone(), "planes": torch.zeros(elems, dtype=torch.uint8, device="cuda")}
    dtable, ptable, npb = s.table, sp.table, ctypes.c_longlong(pbytes)

    def idct_dense(st_):
        L.check(lib.fv_jpeg_idct(L.ptr(st_["coef"]), ne, L.ptr(dtable), L.ptr(st_["planes"]), ne, b, L.stream_of(st_["planes"])), "fv_jpeg_idct")

    def idct_packed(st_):
        L.check(lib.fv_jpeg_idct_packed(L.ptr(st_["coef"]), npb, L.ptr(ptable), L.ptr(st_["planes"]), ne, b, L.stream_of(st_["planes"])),
                "fv_jpeg_idct_packed")

    with limited(a.limit, "planes compared"):
        idct_dense(dbase)
        idct_packed(pbase)
        torch.cuda.synchronize()
        same = bool(torch.equal(dbase["planes"], pbase["planes"]))
    say(f"    planes of the two forms, {elems} bytes: {'identical' if same else 'DIFFERENT'}")
    packed["planes_identical"] = same
    say("    HBM-cold IDCT launch (us per launch, each row timed twice), each next to a plain copy of its own bytes:")
    for name, fn, bs, nb_ in (("fv_jpeg_idct", idct_dense, dbase, 3 * elems), ("fv_jpeg_idct_packed", idct_packed, pbase, pbytes + elems)):
        half_ = nb_ // 2
        cb = {"a": torch.randint(0, 256, (half_,), dtype=torch.uint8, device="cuda"), "b": torch.empty(half_, dtype=torch.uint8, device="cuda")}
        for row, f_, base_, names in ((name, fn, bs, ("coef", "planes")), (f"copy of {nb_ / 1e6:.1f} MB", lambda st_: st_["b"].copy_(st_["a"]), cb, ("a", "b"))):
            with limited(a.limit, row):
                fns = rotating(f_, base_, names, nb_, cap=16)
                t = [time_kernel(fns) * 1e6 for _ in range(2)]
                del fns
            packed[row if row == name else name + " copy"] = [round(v, 2) for v in t]
            say(f"        {row:24s}: {t[0]:8.2f} {t[1]:8.2f} us   {nb_ / 1e6:6.1f} MB   {nb_ / min(t) / 1e6:.2f} TB/s")
        del cb
    packed["idct_packed_over_dense"] = round(min(packed["fv_jpeg_idct_packed"]) / min(packed["fv_jpeg_idct"]), 2)
    say(f"        fv_jpeg_idct_packed / fv_jpeg_idct: {packed['idct_packed_over_dense']:.2f}; over their own copies: "
        f"{min(packed['fv_jpeg_idct_packed']) / min(packed['fv_jpeg_idct_packed copy']):.2f} and "
        f"{min(packed['fv_jpeg_idct']) / min(packed['fv_jpeg_idct copy']):.2f}")
    rec["packed"] = packed
    plines = lines[:2] + lines[mark:] + [json.dumps({"batch": B, "size": S, "packed": packed})]
    say(json.dumps(rec))
    for path, text in ((a.log, lines), (a.packed_log, plines)):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
