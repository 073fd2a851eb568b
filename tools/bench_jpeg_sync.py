"""Time the INDEX-FREE JPEG path (fastvim_amd/jpeg.py ``put_jpeg_sync``, csrc/jpeg_sync.hip ``fv_jpeg_sync``) in ONE process, on
the files and crops of tools/bench_jpeg.py (B = 128 synthetic photograph-like files, ``RandomResizedCrop(224)``):

  (a) HOST time per image of ``put_jpeg_sync`` next to ``put_jpeg`` and ``put_jpeg_indexed``, passes alternating, one thread;
  (b) the link: bytes per batch of each path;
  (c) ``fv_jpeg_sync`` HBM-cold (operand sets rotated past the Infinity Cache, bench.py's ``rotating``) at every ``subseq_bytes``
      from 16 to 1024, each twice, with the distribution of rounds per sample; next to it ``fv_jpeg_huff`` at S = 1 and
      ``fv_jpeg_idct`` + ``fv_jpeg_rgb`` on the same batch, and a device copy of the same bytes; the pixels of every
      setting are compared with the dense stage's first;
  (d) what speculation is worth, from the host's serial run of the same passes on the whole images: the share of speculative
      exit states that were INVALID, valid but wrong, and right, and the longest run of INVALID ones.

    python tools/bench_jpeg_sync.py

Every GPU step runs under a time limit of its own (``--limit`` seconds, bench_u8's watchdog).  Reads nothing outside the
repository and sets no threshold.  The log goes to stdout and to ``--log`` (profiles/jpeg_sync_bench.log), the last line
one JSON record."""
import argparse
import ctypes
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
from bench import rotating, time_kernel  # noqa: E402
from bench_jpeg import B, S as SIZE, files  # noqa: E402
from bench_u8 import limited  # noqa: E402
from fastvim_amd import _lib as L  # noqa: E402
from fastvim_amd import jpeg  # noqa: E402
from fastvim_amd.resample import RandomResizedCrop  # noqa: E402

SUBSEQS = (16, 32, 64, 128, 256, 512, 1024)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--limit", type=float, default=120.0, help="seconds each GPU step may take")
    ap.add_argument("--log", default=os.path.join(R, "profiles", "jpeg_sync_bench.log"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    assert torch.cuda.is_available(), "bench_jpeg_sync.py needs a GPU"
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    raws = files(0)
    infos = [jpeg.probe(r) for r in raws]
    random.seed(1)
    rrc = RandomResizedCrop(SIZE, generator=torch.Generator().manual_seed(1))
    draws = [rrc.draw(i.height, i.width) for i in infos]
    file_bytes = sum(map(len, raws))
    S = jpeg.DEFAULT_SEGMENT_MCUS
    say(f"{B} files, {file_bytes / B / 1e3:.1f} KB on average ({file_bytes / 1e6:.2f} MB the batch); S = {S}")
    rec = {"batch": B, "size": SIZE, "file_MB": round(file_bytes / 1e6, 2), "S": S}
    caps = dict(capacity_bytes=B * 600 * 600 * 3 + 16 * B, coef_capacity_bytes=B * 608 * 608 * 6, slots=1)
    dense = jpeg.JpegImageStage(B, SIZE, **caps)
    index = [jpeg.build_index(r, S) for r in raws]

    def put_dense(k):
        i, j, h, w, f = draws[k]
        dense.put_jpeg(k, raws[k], crop=(i, j, h, w), flip=f)

    for k in range(B):
        put_dense(k)
    dense.commit()
    dense.decode()
    torch.cuda.synchronize()
    want = [dense.region(k).clone() for k in range(B)]
    dense_bytes = dense.staged_coef_bytes
    caps["coef_capacity_bytes"] = dense_bytes + 128
    stream_cap = file_bytes + B * (1 << 16)
    indexed = jpeg.JpegImageStage(B, SIZE, stream_capacity_bytes=stream_cap, **caps)
    stages = {Lb: jpeg.JpegImageStage(B, SIZE, stream_capacity_bytes=stream_cap, sync=True, subseq_bytes=Lb, segment_mcus=S, **caps)
              for Lb in SUBSEQS}

    def put_indexed(k):
        i, j, h, w, f = draws[k]
        indexed.put_jpeg_indexed(k, raws[k], index[k], crop=(i, j, h, w), flip=f)

    def put_sync(k, st=stages[jpeg.DEFAULT_SUBSEQ_BYTES]):
        i, j, h, w, f = draws[k]
        st.put_jpeg_sync(k, raws[k], crop=(i, j, h, w), flip=f)

    def put_row(st, fn):
        t0 = time.perf_counter()
        for k in range(B):
            fn(k)
        t = (time.perf_counter() - t0) / B * 1e3
        st.commit()
        torch.cuda.synchronize()
        return t

    # ------------------------------------------------------------------------------------------------------ (a) host
    say("(a) host time per image on one thread, the same files and crops (the minimum of three passes after a warm-up pass; the three "
        "paths alternate):")
    host = {}
    with limited(6 * a.limit, "host rows"):
        rows = {"put_jpeg": (dense, put_dense), "put_jpeg_indexed": (indexed, put_indexed),
                "put_jpeg_sync": (stages[jpeg.DEFAULT_SUBSEQ_BYTES], put_sync)}
        ts = {n: [] for n in rows}
        for _ in range(4):
            for n, (st, fn) in rows.items():
                ts[n].append(put_row(st, fn))
        for n in rows:
            host[n] = round(min(ts[n][1:]), 4)
            say(f"    {n:17s}: {min(ts[n][1:]):7.4f} ms per image (passes: {', '.join(f'{t:.4f}' for t in ts[n])})")
    rec["host_ms_per_image"] = host

    # ------------------------------------------------------------------------------------------------------ (b) link
    sync_stage = stages[jpeg.DEFAULT_SUBSEQ_BYTES]
    assert sync_stage.last_sync_fallbacks == 0
    link = {"dense_MB": round(dense_bytes / 1e6, 2), "indexed_MB": round(indexed.staged_stream_bytes / 1e6, 2),
            "sync_MB": round((sync_stage.staged_stream_bytes + 4 * B * jpeg.SYNC_JOB_INTS) / 1e6, 2)}
    say(f"(b) link bytes per batch: dense coefficients {link['dense_MB']:.2f} MB; indexed stream pool (S = {S}) {link['indexed_MB']:.2f} MB; "
        f"sync stream pool + job table {link['sync_MB']:.2f} MB (tables, reserved entries, the whole scans); the files whole "
        f"{file_bytes / 1e6:.2f} MB")
    rec["link"] = link

    # ---------------------------------------------------------------------------------------------------- (c) device
    lib, b = L.lib(), L.i32(B)
    dev = {}
    say("(c) device, HBM-cold, us per launch (each twice):")
    for Lb in SUBSEQS:
        st = stages[Lb]
        for k in range(B):
            put_sync(k, st)
        st.commit()
        with limited(a.limit, f"pixels subseq_bytes={Lb}"):
            st.decode()
            torch.cuda.synchronize()
            ok = all(torch.equal(st.region(k), want[k]) for k in range(B)) and not bool(st.stream_status().any())
            rounds = st.sync_rounds().numpy()
        s = st._ready
        nsb, nscr = ctypes.c_longlong(st.stream_bytes), ctypes.c_longlong(st.sync_records * jpeg.SYNC_REC_BYTES)
        base = {"stream": s.stream, "sync": s.sync, "scratch": st._sync_scratch}

        def sync(o):
            L.check(lib.fv_jpeg_sync(L.ptr(o["stream"]), nsb, L.ptr(o["sync"]), L.ptr(o["scratch"]), nscr, b, L.stream_of(o["stream"])),
                    "fv_jpeg_sync")
        with limited(a.limit, f"fv_jpeg_sync subseq_bytes={Lb}"):
            # a launch is as long as its slowest sample's rounds -- milliseconds and more, not the microseconds time_kernel's
            # graph of 4 x 32 launches is made for: one pass over the rotated sets between two events, launched eagerly
            fns = rotating(sync, base, ("stream", "sync", "scratch"), st.staged_stream_bytes + st.sync_records * jpeg.SYNC_REC_BYTES, cap=16)
            fns[0]()
            torch.cuda.synchronize()
            t = []
            for _ in range(2):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for fn in fns:
                    fn()
                e1.record()
                torch.cuda.synchronize()
                t.append(e0.elapsed_time(e1) * 1e3 / len(fns))
            del fns
        q = np.percentile(rounds, (0, 50, 90, 100))
        dev[str(Lb)] = {"us": [round(x, 2) for x in t], "rounds_min_median_p90_max": [float(v) for v in q], "identical": bool(ok)}
        say(f"    fv_jpeg_sync subseq_bytes = {Lb:4d}: {t[0]:9.2f} {t[1]:9.2f}; rounds per sample min {q[0]:.0f} median {q[1]:.0f} p90 {q[2]:.0f} "
            f"max {q[3]:.0f}; subsequences per sample median {np.median(s.sjobs[:, 16]):.0f}; pixels and status "
            f"{'identical to the dense path' if ok else 'DIFFERENT'}")
    st = sync_stage
    s = st._ready
    ne, nsb = ctypes.c_longlong(st.coef_elems), ctypes.c_longlong(st.stream_bytes)
    elems = st.coef_elems - s.jtop
    base = {"stream": s.stream, "stable": s.stable, "coef": s.coef}

    def huff(o):
        L.check(lib.fv_jpeg_huff(L.ptr(o["stream"]), nsb, L.ptr(o["stable"]), L.ptr(o["coef"]), ne, b, L.stream_of(o["coef"])), "fv_jpeg_huff")
    with limited(a.limit, "fv_jpeg_huff"):
        fns = rotating(huff, base, ("stream", "stable", "coef"), st.staged_stream_bytes + 2 * elems, cap=16)
        t = [time_kernel(fns) * 1e6 for _ in range(2)]
        del fns
    dev["huff"] = [round(x, 2) for x in t]
    say(f"    fv_jpeg_huff at S = {S} on the entries fv_jpeg_sync made: {t[0]:9.2f} {t[1]:9.2f}")
    nb = ctypes.c_longlong(st.capacity)
    base = {"coef": s.coef, "planes": st._planes, "pool": s.pool}

    def both(o):
        L.check(lib.fv_jpeg_idct(L.ptr(o["coef"]), ne, L.ptr(s.table), L.ptr(o["planes"]), ne, b, L.stream_of(o["pool"])), "fv_jpeg_idct")
        L.check(lib.fv_jpeg_rgb(L.ptr(o["planes"]), ne, L.ptr(s.table), L.ptr(o["pool"]), nb, b, L.stream_of(o["pool"])), "fv_jpeg_rgb")
    with limited(a.limit, "idct + rgb"):
        fns = rotating(both, base, ("coef", "planes", "pool"), 3 * st.coef_elems + st.capacity, cap=3)
        t = [time_kernel(fns) * 1e6 for _ in range(2)]
        del fns
    dev["idct_rgb"] = [round(x, 2) for x in t]
    say(f"    fv_jpeg_idct + fv_jpeg_rgb on the same batch: {t[0]:9.2f} {t[1]:9.2f}")
    n = st.staged_stream_bytes
    base = {"src": s.stream, "dst": torch.empty_like(s.stream)}

    def copy(o):
        o["dst"][:n].copy_(o["src"][:n])
    with limited(a.limit, "copy"):
        fns = rotating(copy, base, ("src", "dst"), 2 * n, cap=16)
        t = [time_kernel(fns) * 1e6 for _ in range(2)]
        del fns
    dev["copy"] = [round(x, 2) for x in t]
    best = min(SUBSEQS, key=lambda Lb: min(dev[str(Lb)]["us"]))
    total = min(dev[str(best)]["us"]) + min(dev["huff"]) + min(dev["idct_rgb"])
    say(f"    a device copy of the staged stream bytes ({n / 1e6:.2f} MB): {t[0]:9.2f} {t[1]:9.2f}")
    say(f"    lowest fv_jpeg_sync: subseq_bytes = {best}; sync + huff + idct + rgb = {total:.2f} us, {total / min(dev['copy']):.1f} x the copy, "
        f"{total / 5000:.3f} of a 5 ms FastVim-T step")
    dev["best_subseq_bytes"] = best
    rec["device"] = dev

    # ----------------------------------------------------------------------------------- (d) what speculation is worth
    say("(d) speculation, whole images, the host's serial run of the same passes (fv_jpeg_sync_host, job words [26..28]): of all "
        "subsequences but each file's last, the speculative exit states that were INVALID, valid but not the final state, and "
        "right; the longest run of INVALID ones in a file; rounds:")
    spec = {}
    for Lb in SUBSEQS:
        jobs = np.stack([jpeg.sync_stage(r, None, S, Lb)[2] for r in raws])
        assert not jobs[:, 24].any()
        n = int(jobs[:, 16].sum()) - B
        dead, wrong = int(jobs[:, 26].sum()), int(jobs[:, 27].sum())
        spec[str(Lb)] = {"invalid": round(dead / n, 4), "wrong": round(wrong / n, 4), "right": round(1 - (dead + wrong) / n, 4),
                         "longest_invalid_run": int(jobs[:, 28].max()), "rounds_max": int(jobs[:, 25].max())}
        say(f"    subseq_bytes = {Lb:4d}: INVALID {dead / n:.3f}, valid but wrong {wrong / n:.3f}, right {1 - (dead + wrong) / n:.3f} of {n}; "
            f"longest INVALID run {int(jobs[:, 28].max())}; rounds median {np.median(jobs[:, 25]):.0f} max {int(jobs[:, 25].max())}")
    rec["speculation"] = spec
    say(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    with open(a.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
