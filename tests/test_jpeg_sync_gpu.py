"""The index-free JPEG path on the device (fastvim_amd/jpeg.py ``put_jpeg_sync``, csrc/jpeg_sync.hip ``fv_jpeg_sync``): the
entries a workgroup per sample writes against the serial builder's (``jpeg.build_index``), the coefficients ``fv_jpeg_huff``
then decodes against the host decoder's, the pixels against PIL's, the resampled batch against the ``put_jpeg`` stage's,
mixed batches, a replayed graph, the fallback, and the stages without ``sync=True`` left as they were.  Every comparison is
exact.

Fixtures are at most 64 x 80 and a batch is 8 samples -- files tools/jpeg_sync_check.cpp has taken through the same core
text under the sanitizers.  At 16-byte subsequences the quality-100 noise files have more subsequences than a workgroup
has lanes and need more than two rounds; at 128 bytes the small files have fewer subsequences than lanes, one of them a
single one."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CASES, _INDEX, _WANT = None, {}, {}
SENTINEL = 0x5A5A
LANES = 256                   # SYNC_THREADS of csrc/jpeg_sync.hip


def cases():
    global _CASES
    if _CASES is None:
        _CASES = {}
        for npz in ("jpeg_cases.npz", "jpeg_index_cases.npz"):
            z = np.load(os.path.join(GOLDEN, npz))
            _CASES.update({str(n): (z["jpg_" + str(n)].tobytes(), z["rgb_" + str(n)]) for n in z["names"]})
    return _CASES


def noise100():
    return sorted(n for n in cases() if "_q100_noise_s" in n)


def index(name, S):
    from fastvim_amd import jpeg
    if (name, S) not in _INDEX:
        _INDEX[(name, S)] = jpeg.build_index(cases()[name][0], S)
    return _INDEX[(name, S)]


def _stage(S=1, L=128, batch=8, slots=1, stream=1 << 19, **kw):
    from fastvim_amd.jpeg import JpegImageStage
    return JpegImageStage(batch, 16, capacity_bytes=1 << 20, coef_capacity_bytes=1 << 20, slots=slots, stream_capacity_bytes=stream,
                          sync=True, subseq_bytes=L, segment_mcus=S, **kw)


def batch_a():
    """(fixture, crop, out_full, window, flip)"""
    q = noise100()
    return [("64x80_444_q90_noise", None, None, (0, 0), False),
            ("64x80_422_q90_noise", (13, 21, 33, 35), (24, 24), (4, 8), True),
            ("64x80_420_q90_noise", (5, 9, 40, 50), None, (0, 0), True),
            ("64x80_gray_q90_noise", (31, 0, 2, 80), None, (0, 0), False),
            ("33x47_420_opt_noise", None, (20, 28), (2, 3), False),
            ("33x47_444_opt_noise", (3, 5, 11, 13), None, (0, 0), False),
            (q[0], (15, 31, 2, 2), None, (0, 0), True),                             # a window of very few MCUs
            (q[-1], None, None, (0, 0), False)]


def batch_b():
    q = noise100()
    return [("33x47_gray_opt_noise", None, None, (0, 0), True),
            ("33x47_422_opt_noise", (17, 19, 9, 7), None, (0, 0), False),
            (q[-1], (9, 63, 21, 17), None, (0, 0), False),
            ("64x80_420_q90_noise", None, (32, 40), (16, 24), False),
            ("17x23_420_q75_noise", None, None, (0, 0), False),
            ("8x8_gray_q75_noise", None, None, (0, 0), False),
            ("64x80_444_q90_noise", (47, 3, 17, 9), None, (0, 0), True),
            ("1x1_420_q20_smooth", None, None, (0, 0), False)]


BATCHES = {"a": batch_a, "b": batch_b}


def _put(stage, batch, S, how="sync"):
    """``how``: "sync", "jpeg", or a per-sample list of "sync" / "indexed" / "jpeg" / "array"."""
    for k, (n, crop, out_full, window, flip) in enumerate(batch):
        raw, rgb = cases()[n]
        h = how if isinstance(how, str) else how[k]
        if h == "sync":
            stage.put_jpeg_sync(k, raw, crop=crop, out_full=out_full, window=window, flip=flip)
        elif h == "indexed":
            stage.put_jpeg_indexed(k, raw, index(n, S), crop=crop, out_full=out_full, window=window, flip=flip)
        elif h == "jpeg":
            stage.put_jpeg(k, raw, crop=crop, out_full=out_full, window=window, flip=flip)
        else:
            stage.put(k, rgb, crop=crop, out_full=out_full, window=window, flip=flip)
    stage.commit()


def want(which):
    """The resampled batch of the ``put_jpeg`` stage (the parent's code path), once per batch."""
    if which not in _WANT:
        from fastvim_amd.jpeg import JpegImageStage
        st = JpegImageStage(8, 16, capacity_bytes=1 << 20, coef_capacity_bytes=1 << 20, slots=1)
        _put(st, BATCHES[which](), 0, how="jpeg")
        out = torch.full((8, 3, 16, 16), 77, dtype=torch.uint8, device="cuda")
        st.resample(out=out)
        assert st.last_jpeg_fallbacks == 0
        _WANT[which] = out.cpu()
    return _WANT[which]


@pytest.mark.parametrize("L", [16, 128])
@pytest.mark.parametrize("S", [1, 3, 1000])
@pytest.mark.parametrize("which", ["a", "b"])
def test_entries_coefficients_pixels_status(S, L, which):
    from fastvim_amd import jpeg
    batch = BATCHES[which]()
    assert {n.split("_")[1] for n, *_ in batch_a() + batch_b()} == {"444", "422", "420", "gray"}
    stage = _stage(S, L)
    for s in stage._slots:
        s.coef.fill_(SENTINEL)                             # every coefficient of a window is WRITTEN, zeros included
        s.pool.fill_(0xA5)
    _put(stage, batch, S)
    assert stage.staged_coef_bytes == 0 and stage.staged_stream_bytes > 0      # no coefficient crossed the link
    stage.decode()
    torch.cuda.synchronize()
    assert stage.last_jpeg_fallbacks == 0 and stage.last_fallbacks == 0 and stage.last_sync_fallbacks == 0
    assert torch.equal(stage.stream_status(), torch.zeros(8, dtype=torch.int32))
    s = stage._ready
    jobs, rounds = s.sync.cpu().numpy().reshape(8, 32), stage.sync_rounds().numpy()
    subseqs = s.sjobs[:, 16]
    assert np.array_equal(jobs[:, :24], s.sjobs[:, :24]) and np.array_equal(jobs[:, 25], rounds) and (jobs[:, 26:] == 0).all()
    if L == 16:
        assert subseqs.max() > LANES and rounds.max() > 2  # the strided loops, and a fixed point of many rounds
    else:
        assert subseqs.max() < LANES
        assert which == "a" or subseqs.min() == 1          # batch b holds a file of a single subsequence
    assert (rounds <= subseqs).all()
    pool, coef = s.stream.cpu().numpy(), s.coef.cpu().numpy()
    rest = np.ones(coef.size, bool)
    top = coef.size
    for k, (n, crop, *_) in enumerate(batch):
        raw, rgb = cases()[n]
        info = jpeg.probe(raw)
        win = jpeg.mcu_window(info.height, info.width, info.subsampling, crop)
        # the entries: the serial builder's for the same groups, byte for byte
        ent = np.frombuffer(index(n, S), np.uint8)[jpeg.INDEX_HEAD_BYTES:].reshape(-1, 16)
        mx = jpeg._probe(raw)[6]
        gpr, gx0, gw = -(-mx // S), int(jobs[k, 8]), int(jobs[k, 9])
        assert (gx0, gw) == (win[0] // S, (win[0] + win[2] - 1) // S - win[0] // S + 1)
        e_want = np.stack([ent[(win[1] + y) * gpr + gx0:(win[1] + y) * gpr + gx0 + gw] for y in range(win[3])])
        eoff = int(jobs[k, 17])
        assert np.array_equal(pool[eoff:eoff + 16 * gw * win[3]].reshape(win[3], gw, 16), e_want), (n, S, L)
        # the device changed nothing else of the sample's region: tables and scan as the host staged them
        lo, hi = int(jobs[k, 19]), int(jobs[k, 10]) + int(jobs[k, 12])
        host = s.stream_pin.numpy()
        assert np.array_equal(pool[lo:eoff], host[lo:eoff]) and np.array_equal(pool[eoff + 16 * gw * win[3]:hi], host[eoff + 16 * gw * win[3]:hi])
        rec, ref = jpeg.entropy_decode(raw, win)
        base = jpeg._rec_i64(s.records[k], 9)
        assert base + ref.size == top, (k, base, ref.size, top)          # reserved from the top downward, nothing between
        top = base
        assert np.array_equal(coef[base:base + ref.size], ref), (n, S, L, int((coef[base:base + ref.size] != ref).sum()))
        rest[base:base + ref.size] = False
        t, l, h, w = (0, 0, info.height, info.width) if crop is None else crop
        assert torch.equal(stage.region(k).cpu(), torch.from_numpy(np.ascontiguousarray(rgb[t:t + h, l:l + w]))), (n, S, L)
    assert (coef[rest] == SENTINEL).all(), int((coef[rest] != SENTINEL).sum())


@pytest.mark.parametrize("L", [16, 128])
def test_resample_equals_the_put_jpeg_stage(L):
    for S in (1, 3, 1000):
        for which in ("a", "b"):
            stage = _stage(S, L, slots=2)
            _put(stage, BATCHES[which](), S)
            out = torch.full((8, 3, 16, 16), 99, dtype=torch.uint8, device="cuda")
            stage.resample(out=out)
            assert stage.last_jpeg_fallbacks == 0 and stage.last_sync_fallbacks == 0 and stage.staged_coef_bytes == 0
            assert torch.equal(out.cpu(), want(which)), (S, L, [(k, int((out.cpu()[k] != want(which)[k]).sum())) for k in range(8)])
            assert torch.equal(stage.stream_status(), torch.zeros(8, dtype=torch.int32))


def test_mixed_batch_of_arrays_files_indexed_and_sync_files():
    how = ["sync", "jpeg", "array", "indexed", "sync", "indexed", "array", "sync"]
    stage = _stage(3, 64, slots=2)
    _put(stage, batch_a(), 3, how=how)
    s = stage._ready
    assert [int(j) for j in s.sjobs[:, 0]] == [1, 0, 0, 0, 1, 0, 0, 1]          # slots without a job: the workgroup returns at once
    assert [int(j) for j in s.srecords[:, 0]] == [1, 0, 0, 1, 1, 1, 0, 1]
    out = torch.full((8, 3, 16, 16), 99, dtype=torch.uint8, device="cuda")
    stage.resample(out=out)
    assert stage.last_jpeg_fallbacks == 0 and stage.last_sync_fallbacks == 0
    assert torch.equal(out.cpu(), want("a"))
    assert torch.equal(stage.stream_status(), torch.zeros(8, dtype=torch.int32))
    rounds = stage.sync_rounds()
    assert all(int(rounds[k]) == 0 for k in range(8) if how[k] != "sync")


def test_graph_replay_syncs_the_batch_of_the_moment():
    stage = _stage(3, 64, slots=1)
    x = torch.zeros(8, 3, 16, 16, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _put(stage, batch_a(), 3)
        stage.resample(out=x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), want("a"))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stage.resample(out=x)
    # other files and windows at the same pool addresses: entries of the batch before would show.  The entry region is
    # filled again by every commit, so fv_jpeg_huff can only start from what fv_jpeg_sync wrote in this replay
    for which in ("b", "a", "b"):
        _put(stage, BATCHES[which](), 3)
        graph.replay()
        assert torch.equal(x.cpu(), want(which)), (which, [(k, int((x.cpu()[k] != want(which)[k]).sum())) for k in range(8)])
        assert torch.equal(stage.stream_status(), torch.zeros(8, dtype=torch.int32))


def test_a_refused_file_takes_the_put_jpeg_route():
    refused = sorted(n for n in cases() if "_rst" in n)[:2] + ["33x47_420_progressive"]
    batch = [(n, None, None, (0, 0), False) for n in refused] + batch_b()[:5]
    stage = _stage(1, 128)
    _put(stage, batch, 1)
    assert stage.last_sync_fallbacks == 3 and stage.last_jpeg_fallbacks == 1      # the progressive file is PIL's in put_jpeg too
    assert [int(j) for j in stage._ready.sjobs[:, 0]] == [0, 0, 0, 1, 1, 1, 1, 1]
    stage.decode()
    for k, (n, crop, *_) in enumerate(batch):
        rgb = cases()[n][1]
        t, l, h, w = (0, 0, *rgb.shape[:2]) if crop is None else crop
        assert torch.equal(stage.region(k).cpu(), torch.from_numpy(np.ascontiguousarray(rgb[t:t + h, l:l + w]))), n
    assert torch.equal(stage.stream_status(), torch.zeros(8, dtype=torch.int32))
    # a scan above max_scan_bytes is such a file too
    small = _stage(1, 128, max_scan_bytes=512)
    _put(small, batch_b(), 1)
    scans = [int(j[12]) for j in _stage_jobs(batch_b())]
    assert small.last_sync_fallbacks == sum(n > 512 for n in scans) > 0
    out = torch.full((8, 3, 16, 16), 99, dtype=torch.uint8, device="cuda")
    small.resample(out=out)
    assert torch.equal(out.cpu(), want("b"))


def _stage_jobs(batch):
    from fastvim_amd import jpeg
    return [jpeg.sync_stage(cases()[n][0], run=False)[2] for n, *_ in batch]


def test_stages_without_sync_launch_what_they_launched():
    from fastvim_amd import _lib as L
    from fastvim_amd.jpeg import JpegImageStage
    names = ("fv_jpeg_sync", "fv_jpeg_huff", "fv_jpeg_idct", "fv_jpeg_idct_packed", "fv_jpeg_rgb")
    lib = L.lib()
    real = {name: getattr(lib, name) for name in names}

    def launches_of(stage, how, S):
        seen = []
        try:
            for name, fn in real.items():
                lib._wrapped[name] = lambda *a, _n=name, _f=fn: (seen.append(_n), _f(*a))[1]
            _put(stage, batch_a(), S, how=how)
            out = torch.full((8, 3, 16, 16), 99, dtype=torch.uint8, device="cuda")
            stage.resample(out=out)
        finally:
            lib._wrapped.update(real)
        return seen, out.cpu()

    dense = JpegImageStage(8, 16, capacity_bytes=1 << 20, coef_capacity_bytes=1 << 20, slots=1)
    assert not dense.sync and not hasattr(dense._slots[0], "sync") and not hasattr(dense, "_sync_scratch")
    seen, out = launches_of(dense, "jpeg", 0)
    assert seen == ["fv_jpeg_idct", "fv_jpeg_rgb"] and torch.equal(out, want("a"))
    indexed = JpegImageStage(8, 16, capacity_bytes=1 << 20, coef_capacity_bytes=1 << 20, slots=1, stream_capacity_bytes=1 << 19)
    assert not indexed.sync and not hasattr(indexed._slots[0], "sync")
    seen, out = launches_of(indexed, "indexed", 3)
    assert seen == ["fv_jpeg_huff", "fv_jpeg_idct", "fv_jpeg_rgb"] and torch.equal(out, want("a"))
    with pytest.raises(RuntimeError, match="sync=True"):
        indexed.put_jpeg_sync(0, cases()["8x8_gray_q75_noise"][0])
    with pytest.raises(RuntimeError):
        indexed.sync_rounds()
    seen, out = launches_of(_stage(3, 64), "sync", 3)
    assert seen == ["fv_jpeg_sync", "fv_jpeg_huff", "fv_jpeg_idct", "fv_jpeg_rgb"] and torch.equal(out, want("a"))


def test_arguments_and_refusals():
    from fastvim_amd.jpeg import JpegImageStage
    kw = dict(capacity_bytes=1 << 20, coef_capacity_bytes=1 << 20)
    with pytest.raises(ValueError, match="packed"):
        JpegImageStage(8, 16, coef_format="packed", sync=True, **kw)
    with pytest.raises(ValueError, match="stream_capacity_bytes"):
        JpegImageStage(8, 16, sync=True, **kw)
    for L in (8, 24, 2048):
        with pytest.raises(ValueError, match="power of two"):
            JpegImageStage(8, 16, stream_capacity_bytes=1 << 16, sync=True, subseq_bytes=L, **kw)
    for extra in (dict(subseq_bytes=64), dict(max_scan_bytes=1 << 16), dict(segment_mcus=2)):
        with pytest.raises(ValueError, match="belong to sync=True"):
            JpegImageStage(8, 16, stream_capacity_bytes=1 << 16, **extra, **kw)
    assert _stage(1, 16).max_scan_bytes == 16384 * 16 and _stage(1, 1024).max_scan_bytes == 1 << 20      # the cap on subsequences
    raw = cases()["64x80_420_q90_noise"][0]
    stage = _stage(1, 128)
    from fastvim_amd import jpeg
    assert stage.subseq_bytes == 128 and _stage(1, None).subseq_bytes == jpeg.DEFAULT_SUBSEQ_BYTES == 128      # the default
    with pytest.raises(ValueError, match="does not lie inside"):
        stage.put_jpeg_sync(0, raw, crop=(0, 0, 65, 80))
    small = _stage(1, 128, stream=4096)
    with pytest.raises(ValueError, match="stream_capacity_bytes"):
        small.put_jpeg_sync(0, raw)
    # a refusal leaves the sample free: the same slot is then put for real, and the batch decodes
    for k in range(8):
        stage.put_jpeg_sync(k, raw, crop=(8 * k, 0, 8, 80))
    with pytest.raises(ValueError, match="already put"):
        stage.put_jpeg_sync(3, raw)
    stage.commit()
    stage.decode()
    rgb = cases()["64x80_420_q90_noise"][1]
    for k in range(8):
        assert torch.equal(stage.region(k).cpu(), torch.from_numpy(np.ascontiguousarray(rgb[8 * k:8 * k + 8])))
    assert torch.equal(stage.stream_status(), torch.zeros(8, dtype=torch.int32))
