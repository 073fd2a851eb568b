"""Time the INDEXED JPEG path (fastvim_amd/jpeg.py ``put_jpeg_indexed``, csrc/jpeg.hip ``fv_jpeg_huff``) in ONE process, on the
files and crops of tools/bench_jpeg.py (B = 128 synthetic photograph-like files, ``RandomResizedCrop(224)``):

  (a) HOST time per image of ``put_jpeg_indexed`` next to dense ``put_jpeg`` (the parent's code), passes alternating, on one
      thread and on several, each row twice;
  (b) the link: bytes per batch of the stream pool (tables + index entries + file bytes) and the stream table, next to the
      dense and the packed coefficients of the same batch;
  (c) ``fv_jpeg_huff`` HBM-cold (operand sets rotated past the Infinity Cache, bench.py's ``rotating``) for S in
      {1, 2, 4, 8, 16, whole row}, each twice, next to ``fv_jpeg_idct`` + ``fv_jpeg_rgb`` on the same batch; the pixels of
      every S are compared with the dense stage's first;
  (d) index bytes per file for every S, and the one-off ``build_index`` time.

    python tools/bench_jpeg_index.py

Every GPU step runs under a time limit of its own (``--limit`` seconds, bench_u8's watchdog).  Reads nothing outside the
repository and sets no threshold.  The log goes to stdout and to ``--log`` (profiles/jpeg_index_bench.log), the last line
one JSON record."""
import argparse
import ctypes
import json
import os
import random
import sys
import time
from concurrent.futures import ThreadPoolExecutor

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))
import numpy as np  # noqa: E402,F401
import torch  # noqa: E402
import fastvim_amd  # noqa: E402,F401  (sets the graph-capture switch before HIP initialises)
from bench import rotating, time_kernel  # noqa: E402
from bench_jpeg import B, S as SIZE, files  # noqa: E402
from bench_u8 import limited  # noqa: E402
from fastvim_amd import _lib as L  # noqa: E402
from fastvim_amd import jpeg  # noqa: E402
from fastvim_amd.resample import RandomResizedCrop  # noqa: E402

ROW = 8192                    # S of "whole row": no image has more MCUs in a row
SEGMENTS = (1, 2, 4, 8, 16, ROW)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--limit", type=float, default=120.0, help="seconds each GPU step may take")
    ap.add_argument("--threads", type=int, default=8, help="loader threads of the multi-thread rows")
    ap.add_argument("--log", default=os.path.join(R, "profiles", "jpeg_index_bench.log"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    assert torch.cuda.is_available(), "bench_jpeg_index.py needs a GPU"
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    raws = files(0)
    infos = [jpeg.probe(r) for r in raws]
    random.seed(1)
    rrc = RandomResizedCrop(SIZE, generator=torch.Generator().manual_seed(1))
    draws = [rrc.draw(i.height, i.width) for i in infos]
    file_bytes = sum(map(len, raws))
    say(f"{B} files, {file_bytes / B / 1e3:.1f} KB on average ({file_bytes / 1e6:.2f} MB the batch); default S = {jpeg.DEFAULT_SEGMENT_MCUS}")
    rec = {"batch": B, "size": SIZE, "file_MB": round(file_bytes / 1e6, 2), "default_S": jpeg.DEFAULT_SEGMENT_MCUS}
    caps = dict(capacity_bytes=B * 600 * 600 * 3 + 16 * B, coef_capacity_bytes=B * 608 * 608 * 6, slots=1)
    dense = jpeg.JpegImageStage(B, SIZE, **caps)

    # ------------------------------------------------------------------------------------------------- (d) the index
    say("(d) the index: bytes per file (header and tables 6592, 16 per group) and the one-off build_index time:")
    index, sizes = {}, {}
    for S in SEGMENTS:
        t0 = time.perf_counter()
        index[S] = [jpeg.build_index(r, S) for r in raws]
        t = (time.perf_counter() - t0) / B * 1e3
        sizes[S] = sum(map(len, index[S])) / B
        say(f"    S = {S if S != ROW else 'row':>4}: {sizes[S] / 1e3:7.2f} KB per file ({sizes[S] * B / file_bytes:.2f} of the files' bytes), "
            f"build_index {t:.3f} ms per file")
        rec.setdefault("index", {})[str(S)] = {"KB_per_file": round(sizes[S] / 1e3, 2), "build_ms": round(t, 3)}

    def put_dense(k):
        i, j, h, w, f = draws[k]
        dense.put_jpeg(k, raws[k], crop=(i, j, h, w), flip=f)

    # the indexed stage's coefficient pool holds this batch's windows and no more: its operand sets are cloned whole below
    for k in range(B):
        put_dense(k)
    dense.commit()
    torch.cuda.synchronize()
    caps["coef_capacity_bytes"] = dense.staged_coef_bytes + 128
    stage = jpeg.JpegImageStage(B, SIZE, stream_capacity_bytes=file_bytes + B * (1 << 16), **caps)

    def put_indexed(k, S=jpeg.DEFAULT_SEGMENT_MCUS):
        i, j, h, w, f = draws[k]
        stage.put_jpeg_indexed(k, raws[k], index[S][k], crop=(i, j, h, w), flip=f)

    def put_row(st, fn, threads):
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

    # ------------------------------------------------------------------------------------------------------ (a) host
    say(f"(a) host time per image, S = {jpeg.DEFAULT_SEGMENT_MCUS}, the same files and crops (each row: the minimum of three passes after a "
        "warm-up pass; dense and indexed passes alternate; every row twice):")
    host = {}
    with limited(6 * a.limit, "host rows"):
        for threads in (1, a.threads):
            for rep in (1, 2):
                td, ti = [], []
                for _ in range(4):
                    td.append(put_row(dense, put_dense, threads))
                    ti.append(put_row(stage, put_indexed, threads))
                for name, ts in (("put_jpeg", td[1:]), ("put_jpeg_indexed", ti[1:])):
                    host.setdefault(f"{name}_{threads}", []).append(round(min(ts), 4))
                    say(f"    {name:17s} {threads:2d} thread(s), row {rep}: {min(ts):7.4f} ms per image (passes: {', '.join(f'{t:.4f}' for t in ts)})")
            r = min(host[f"put_jpeg_indexed_{threads}"]) / min(host[f"put_jpeg_{threads}"])
            say(f"    put_jpeg_indexed / put_jpeg on {threads} thread(s): {r:.3f}")
            host[f"ratio_{threads}"] = round(r, 3)
    rec["host_ms_per_image"] = host
    with limited(a.limit, "copy of the staged bytes"):      # what the host time is expected to fall to: a copy of the bytes
        src = [np.frombuffer(r, np.uint8) for r in raws]
        dst = np.empty(max(map(len, raws)), np.uint8)
        ts = []
        for _ in range(4):
            t0 = time.perf_counter()
            for x in src:
                np.copyto(dst[:x.size], x)
            ts.append((time.perf_counter() - t0) / B * 1e3)
        say(f"    a numpy copy of every WHOLE file, for scale: {min(ts[1:]):.4f} ms per image")
        host["copy_whole_file"] = round(min(ts[1:]), 4)

    # ------------------------------------------------------------------------------------------------------ (b) link
    for k in range(B):
        put_dense(k)
    dense.commit()
    pst = jpeg.JpegImageStage(B, SIZE, capacity_bytes=caps["capacity_bytes"], coef_capacity_bytes=B * 608 * 608, slots=1,
                              coef_format="packed", plane_capacity_bytes=B * 608 * 608 * 3)
    for k in range(B):
        i, j, h, w, f = draws[k]
        pst.put_jpeg(k, raws[k], crop=(i, j, h, w), flip=f)
    pst.commit()
    torch.cuda.synchronize()
    dense_bytes, packed_bytes = dense.staged_coef_bytes, pst.staged_coef_bytes
    del pst
    table_bytes = 4 * int(L.lib().fv_jpeg_stream_table_ints(L.i32(B)))
    say(f"(b) link bytes per batch: dense coefficients {dense_bytes / 1e6:.2f} MB, packed {packed_bytes / 1e6:.2f} MB, the files whole "
        f"{file_bytes / 1e6:.2f} MB; indexed = stream pool (4 tables of 5696 bytes + 16 per group + the file bytes of the window's "
        f"groups) + stream table ({table_bytes} bytes):")
    link = {"dense_MB": round(dense_bytes / 1e6, 2), "packed_MB": round(packed_bytes / 1e6, 2)}
    want = None
    dev = {}
    lib, b = L.lib(), L.i32(B)
    dense.decode()
    torch.cuda.synchronize()
    want = [dense.region(k).clone() for k in range(B)]
    for S in SEGMENTS:
        for k in range(B):
            put_indexed(k, S)
        stage.commit()
        s = stage._ready
        lanes = int(s.stable_np[B * jpeg.SREC_INTS + B])
        sb = stage.staged_stream_bytes
        link[str(S)] = {"stream_MB": round(sb / 1e6, 3), "lanes": lanes}
        say(f"    S = {S if S != ROW else 'row':>4}: {(sb + table_bytes) / 1e6:6.2f} MB ({lanes} groups; tables {B * 5696 / 1e6:.2f}, entries "
            f"{16 * lanes / 1e6:.2f}, file bytes {(sb - B * 5696 - 16 * lanes) / 1e6:.2f}): {(sb + table_bytes) / dense_bytes:.3f} of dense, "
            f"{(sb + table_bytes) / packed_bytes:.3f} of packed")
        # ------------------------------------------------------------------------------------------------ (c) device
        with limited(a.limit, f"pixels S={S}"):
            stage.decode()
            torch.cuda.synchronize()
            same = all(torch.equal(stage.region(k), want[k]) for k in range(B)) and not bool(stage.stream_status().any())
            assert stage.last_jpeg_fallbacks == 0 and stage.staged_coef_bytes == 0
        elems = stage.coef_elems - s.jtop
        base = {"stream": s.stream, "stable": s.stable, "coef": s.coef}
        nsb, ne = ctypes.c_longlong(stage.stream_bytes), ctypes.c_longlong(stage.coef_elems)

        def huff(st_):
            L.check(lib.fv_jpeg_huff(L.ptr(st_["stream"]), nsb, L.ptr(st_["stable"]), L.ptr(st_["coef"]), ne, b, L.stream_of(st_["coef"])),
                    "fv_jpeg_huff")
        with limited(a.limit, f"fv_jpeg_huff S={S}"):
            fns = rotating(huff, base, ("stream", "stable", "coef"), sb + 2 * elems, cap=16)
            t = [time_kernel(fns) * 1e6 for _ in range(2)]
            del fns
            ok = same and not bool(stage.stream_status().any())
        dev[str(S)] = [round(x, 2) for x in t]
        say(f"          fv_jpeg_huff HBM-cold: {t[0]:8.2f} {t[1]:8.2f} us per launch ({lanes} lanes, {2 * elems / 1e6:.1f} MB of coefficients "
            f"written); pixels and status {'identical to the dense path' if ok else 'DIFFERENT'}")
        link[str(S)]["identical"] = ok
    rec["link"] = link
    # the two dense launches on the same batch, for scale
    s = stage._ready
    elems_all = stage.coef_elems
    ne_all, nb = ctypes.c_longlong(elems_all), ctypes.c_longlong(stage.capacity)
    base = {"coef": s.coef, "planes": stage._planes, "pool": s.pool}

    def both(st_):
        L.check(lib.fv_jpeg_idct(L.ptr(st_["coef"]), ne_all, L.ptr(s.table), L.ptr(st_["planes"]), ne_all, b, L.stream_of(st_["pool"])), "fv_jpeg_idct")
        L.check(lib.fv_jpeg_rgb(L.ptr(st_["planes"]), ne_all, L.ptr(s.table), L.ptr(st_["pool"]), nb, b, L.stream_of(st_["pool"])), "fv_jpeg_rgb")
    with limited(a.limit, "idct + rgb"):
        fns = rotating(both, base, ("coef", "planes", "pool"), 3 * stage.coef_elems + stage.capacity, cap=3)
        t = [time_kernel(fns) * 1e6 for _ in range(2)]
        del fns
    dev["idct_rgb"] = [round(x, 2) for x in t]
    say(f"    fv_jpeg_idct + fv_jpeg_rgb on the same batch: {t[0]:8.2f} {t[1]:8.2f} us (three operand sets of the pools' full capacity)")
    best = {S: min(dev[str(S)]) for S in SEGMENTS}
    spread = max(abs(dev[str(S)][0] - dev[str(S)][1]) for S in SEGMENTS)
    low = min(best.values())
    pick = max(S for S in SEGMENTS if best[S] <= low + spread)
    say(f"(c) fv_jpeg_huff: lowest {low:.2f} us; the run's spread (largest difference of a row's two timings) {spread:.2f} us; the largest S "
        f"within it of the lowest: {pick if pick != ROW else 'row'}; share of a 5 ms FastVim-T step at S = {pick if pick != ROW else 'row'}: "
        f"{best[pick] / 5000:.3f}; fv_jpeg_huff / (idct + rgb): {best[pick] / min(dev['idct_rgb']):.2f}")
    dev["pick"] = pick
    rec["device_us"] = dev
    say(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    with open(a.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
