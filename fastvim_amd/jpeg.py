"""JPEG files straight into the uint8 loaders: the decode of the reference's ``datasets.ImageFolder`` --
``Image.open(path).convert("RGB")``, libjpeg-turbo -- split the way GPU loaders split it.  ENTROPY DECODING STAYS ON THE
HOST: marker parsing and Huffman decoding are serial and branchy (csrc/jpeg_host.cpp, plain C++).  Everything per pixel
runs on the device (csrc/jpeg.hip): dequantisation, the 8 x 8 inverse DCT, fancy chroma upsampling and YCbCr -> RGB, byte
for byte what libjpeg-turbo computes, written into the pixel pool ``fv_resample_u8`` already reads -- the resample
launches run unchanged on it::

    stage = JpegImageStage(B, 224, capacity_bytes=B << 20, coef_capacity_bytes=B << 20)
    for k, raw in enumerate(files):                        # bytes of a .jpg
        info = jpeg.probe(raw)
        i, j, h, w, f = rrc.draw(info.height, info.width); stage.put_jpeg(k, raw, crop=(i, j, h, w), flip=f)
    stage.commit(); stage.resample(out=x_u8)

Only the MCUs the crop needs are kept (``mcu_window``), and Huffman decoding stops after the last of them.  The staged
form is dense int16 coefficients, about 3 bytes per window pixel at 4:2:0 -- the order of the RGB crop it replaces.
``JpegImageStage(..., coef_format="packed")`` stages the PACKED form instead (include/fastvim_hip.h: per block a 64-bit
mask of its non-zero AC terms and those values as int8 or int16), a fifth to a third of the dense bytes on the files
measured in DESIGN.md; ``unpack`` restates the format in numpy.

Served: baseline (SOF0) 8-bit Huffman files with one interleaved scan; grayscale, or YCbCr at 4:4:4, 4:2:2 (2x1) or 4:2:0
(2x2).  A file outside that (progressive, arithmetic, 12-bit, CMYK, RGB-coded, other sampling, several scans, 16-bit
tables), and a file the entropy decoder returns an error for, is decoded by PIL on the host and staged as ``put`` stages
it -- identical by construction; ``last_jpeg_fallbacks`` counts them.

INDEXED FILES (opt-in): a file that is read every epoch can be decoded once into a sidecar index (``build_index``) that
records, for every group of ``segment_mcus`` MCUs, where its bits start and what the DC predictors are there.  A stage
built with ``stream_capacity_bytes`` then takes the FILE BYTES of the crop's groups (``put_jpeg_indexed``) and the device
decodes the Huffman codes too, one lane per group (``fv_jpeg_huff``); the host only copies::

    idx = jpeg.build_index(raw)                            # once per file, kept next to it
    stage = JpegImageStage(B, 224, capacity_bytes=B << 20, coef_capacity_bytes=B << 21, stream_capacity_bytes=B << 17)
    stage.put_jpeg_indexed(k, raw, idx, crop=(i, j, h, w), flip=f)

FILES WITHOUT AN INDEX (opt-in): a stage built with ``sync=True`` takes any ``.jpg`` through ``put_jpeg_sync``.  The host
parses the markers and copies the whole scan; the device finds the group starts itself (``fv_jpeg_sync``: the scan is cut
into subsequences of ``subseq_bytes``, each decoded speculatively and again from its predecessor's exit state until nothing
changes) and writes the entries ``fv_jpeg_huff`` then starts from.  A file the index builder would refuse takes the
``put_jpeg`` route inside the same call::

    stage = JpegImageStage(B, 224, capacity_bytes=B << 20, coef_capacity_bytes=B << 21, stream_capacity_bytes=B << 18, sync=True)
    stage.put_jpeg_sync(k, raw, crop=(i, j, h, w), flip=f)"""
import ctypes
import io
import threading
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from .resample import ALIGN, ImageStage, _pair, resample_ok

REC_INTS = 224            # FV_JPEG_REC_INTS
INFO_INTS = 8             # FV_JPEG_INFO_INTS
S444, S422, S420, GRAY = 0, 1, 2, 3      # FV_JPEG_444 ..: PIL's ``subsampling`` numbers, and 3 for one component
REASONS = ("served", "progressive", "arithmetic coding", "not 8-bit precision", "not 1 or 3 components",
           "not YCbCr (Adobe transform 0 or RGB component ids)", "sampling factors", "several scans",
           "16-bit quantisation tables", "malformed or not a JPEG", "frame type other than SOF0")
ERRORS = {-10: "unserved", -11: "data ends early", -12: "bad Huffman code", -13: "run past 63", -14: "wrong restart marker",
          -15: "coefficient capacity", -16: "window outside the image"}
# the index (include/fastvim_hip.h at THE INDEX)
INDEX_REASONS = REASONS + ("restart interval", "different Huffman tables for the two chroma components")
INDEX_ERRORS = {-15: "capacity", -17: "not an index of this version, or an inconsistent header",
                -18: "the index belongs to another file (size or hash)", -19: "an index entry outside the scan or out of order"}
INDEX_MAGIC, INDEX_VERSION, INDEX_HEAD_BYTES = 0x58494A46, 1, 6592
SREC_INTS = 32            # FV_JPEG_STREAM_REC_INTS
DEFAULT_SEGMENT_MCUS = 1  # S: MCUs per group; the S of the lowest fv_jpeg_huff time in profiles/jpeg_index_bench.log
SYNC_JOB_INTS, SYNC_REC_BYTES = 32, 32    # FV_JPEG_SYNC_JOB_INTS, FV_JPEG_SYNC_REC_BYTES
SYNC_MAX_SUBSEQS = 16384                  # FV_JPEG_SYNC_MAX_SUBSEQS
DEFAULT_SUBSEQ_BYTES = 128                # the subseq_bytes of the lowest fv_jpeg_sync time in profiles/jpeg_sync_bench.log
SYNC_STATUS = {5: "a sync job that does not fit its buffers", 6: "an exit state stays INVALID before the last group start needed"}
SYNC_REFUSALS = (-10, -11, -20)           # unserved or not indexable, fill bytes inside the scan, a scan above max_scan_bytes
_MCU = ((1, 1), (2, 1), (2, 2), (1, 1))  # (h_max, v_max) of a sampling class


class JpegInfo(NamedTuple):
    height: int
    width: int
    subsampling: int      # 0: 4:4:4, 1: 4:2:2, 2: 4:2:0 (PIL's numbers), 3: grayscale, -1: unserved
    served: bool
    reason: str           # "served", or why not (REASONS)


def _as_bytes(data):
    return data if isinstance(data, bytes) else bytes(data)


def _probe(data):
    info = (ctypes.c_int * INFO_INTS)()
    rc = L.host_lib().fv_jpeg_probe(ctypes.c_char_p(data), ctypes.c_longlong(len(data)), info)
    if rc != 0:
        raise RuntimeError(f"fv_jpeg_probe: code {rc}")
    return list(info)


def probe(data):
    """What the header says, and whether the device path serves the file.  Host code of the library: no GPU needed."""
    h, w, _, cls, ok, reason = _probe(_as_bytes(data))[:6]
    return JpegInfo(h, w, cls, bool(ok), REASONS[reason])


def mcu_window(height, width, subsampling, crop=None):
    """The rectangle of MCUs ``(x0, y0, w, h)`` the crop ``(top, left, h, w)`` needs: the crop widened by 2 luma pixels on
    every side where chroma is subsampled -- the fancy upsampler's true neighbour samples at an interior border --
    clamped to the image, then widened to whole MCUs."""
    hmax, vmax = _MCU[subsampling]
    t, l, h, w = (0, 0, height, width) if crop is None else crop
    px, py = 2 * (hmax > 1), 2 * (vmax > 1)
    x0, x1 = max(l - px, 0), min(l + w + px, width)
    y0, y1 = max(t - py, 0), min(t + h + py, height)
    mw, mh = 8 * hmax, 8 * vmax
    return x0 // mw, y0 // mh, -(-x1 // mw) - x0 // mw, -(-y1 // mh) - y0 // mh


def window_elements(subsampling, window):
    """int16 coefficients of a window: 64 per block, h_i * v_i blocks per MCU and component."""
    hmax, vmax = _MCU[subsampling]
    return window[2] * window[3] * 64 * (1 if subsampling == GRAY else hmax * vmax + 2)


def packed_bound(blocks):
    """The worst-case bytes of ``blocks`` blocks in the packed form (``fv_jpeg_packed_bound``)."""
    return int(L.host_lib().fv_jpeg_packed_bound(ctypes.c_longlong(int(blocks))))


def _aligned_bytes(n, align=16):
    """A uint8 array of ``n`` bytes whose first byte is ``align``-byte aligned."""
    raw = np.zeros(n + align, np.uint8)
    lead = -raw.ctypes.data % align
    return raw[lead:lead + n]


def _decode_packed(data, win, out, rec):
    return L.host_lib().fv_jpeg_entropy_decode_packed(ctypes.c_char_p(data), ctypes.c_longlong(len(data)), (ctypes.c_int * 4)(*win),
                                                      ctypes.c_void_p(out.ctypes.data), ctypes.c_longlong(out.size),
                                                      ctypes.c_void_p(rec.ctypes.data))


def _rec_i64(rec, at):
    u = rec.view(np.uint32)
    return int(u[at]) | int(u[at + 1]) << 32


def _rec_add(rec, at, delta):
    u = rec.view(np.uint32)
    v = _rec_i64(rec, at) + delta
    u[at], u[at + 1] = v & 0xffffffff, v >> 32


def unpack(record, packed):
    """The packed form restated in numpy: the dense int16 coefficients (64 per block, natural order, the blocks numbered as
    the dense form numbers them) of the packed ``record`` and the uint8 bytes it describes -- ``packed[0]`` is the byte
    the record's offsets count from.  Raises ``ValueError`` where a header or a value lies outside ``packed``."""
    record, packed = np.asarray(record, np.int32), np.ascontiguousarray(packed, np.uint8)
    if record[0] != 2:
        raise ValueError("unpack: not the record of a packed job")
    blocks, hb, vb = int(record[17]), _rec_i64(record, 25), _rec_i64(record, 27)
    if hb < 0 or hb % 16 or hb + 16 * blocks > packed.size or vb < 0 or vb % 2 or vb > packed.size:
        raise ValueError("unpack: the headers do not lie inside the bytes")
    hdr = packed[hb:hb + 16 * blocks].view("<u4").reshape(blocks, 4)
    dense = np.zeros((blocks, 64), np.int16)
    dense[:, 0] = (hdr[:, 3] & 0xffff).astype(np.uint16).view(np.int16)
    for b in range(blocks):
        mask = (int(hdr[b, 0]) | int(hdr[b, 1]) << 32) & ~1
        ks = [k for k in range(64) if mask >> k & 1]
        wide, off = int(hdr[b, 2]) >> 31, vb + (int(hdr[b, 2]) & 0x7fffffff)
        if off % 2 or off + len(ks) * (1 + wide) > packed.size:
            raise ValueError(f"unpack: the values of block {b} do not lie inside the bytes")
        dense[b, ks] = packed[off:off + len(ks) * (1 + wide)].view("<i2" if wide else np.int8)
    return dense.reshape(-1)


def entropy_decode(data, window=None, packed=False):
    """The host decoder on its own (no GPU): ``(record, coefficients)`` -- the int32 record of ``FV_JPEG_REC_INTS`` words
    and the int16 coefficients of ``window`` (default: the whole image), as include/fastvim_hip.h lays them out.  With
    ``packed=True``: ``(record, bytes)`` of the packed form, the uint8 bytes written (headers, then values).  Raises
    ``ValueError`` with the decoder's reason."""
    data = _as_bytes(data)
    h, w, _, cls, ok, reason, mx, my = _probe(data)
    if not ok:
        raise ValueError(f"fv_jpeg_entropy_decode: unserved file ({REASONS[reason]})")
    win = (0, 0, mx, my) if window is None else tuple(int(v) for v in window)
    if packed:
        out = _aligned_bytes(packed_bound(max(window_elements(cls, win), 0) // 64))
        rec = np.zeros(REC_INTS, np.int32)
        rc = _decode_packed(data, win, out, rec)
        if rc != 0:
            raise ValueError(f"fv_jpeg_entropy_decode_packed: {ERRORS.get(rc, 'error')} (code {rc})")
        return rec, out[:_rec_i64(rec, 15)].copy()
    coef = np.zeros(max(window_elements(cls, win), 0), np.int16)
    rec = np.zeros(REC_INTS, np.int32)
    rc = L.host_lib().fv_jpeg_entropy_decode(ctypes.c_char_p(data), ctypes.c_longlong(len(data)), (ctypes.c_int * 4)(*win),
                                             ctypes.c_void_p(coef.ctypes.data), ctypes.c_longlong(coef.size),
                                             ctypes.c_void_p(rec.ctypes.data))
    if rc != 0:
        raise ValueError(f"fv_jpeg_entropy_decode: {ERRORS.get(rc, 'error')} (code {rc})")
    return rec, coef


class JpegIndexInfo(NamedTuple):
    nbytes: int           # of the file
    hash: int             # FNV-1a 64 of its bytes
    height: int
    width: int
    subsampling: int
    components: int
    mcus_x: int
    mcus_y: int
    segment_mcus: int     # S
    groups_per_row: int
    groups: int
    scan: int             # offset of the first entropy-coded byte


def build_index(raw, segment_mcus=DEFAULT_SEGMENT_MCUS):
    """The index of a JPEG file as ``bytes`` (host code: no GPU needed, no state): per group of ``segment_mcus`` MCUs of
    an MCU row the bit position and the DC predictors, with the tables the device decodes from.  Built once per file and
    kept; ``put_jpeg_indexed`` takes it.  ``ValueError`` with the reason for a file that is not indexed (unserved files,
    restart intervals): those keep ``put_jpeg``."""
    raw, S = _as_bytes(raw), int(segment_mcus)
    if not 1 <= S <= 65536:
        raise ValueError(f"build_index: segment_mcus {S} outside [1, 65536]")
    info = _probe(raw)
    if not info[4]:
        raise ValueError(f"build_index: unserved file ({REASONS[info[5]]})")
    lib = L.host_lib()
    bound = int(lib.fv_jpeg_index_bound(L.i32(info[6]), L.i32(info[7]), L.i32(S)))
    out = np.zeros(max(bound, 16), np.uint8)
    n = int(lib.fv_jpeg_build_index(ctypes.c_char_p(raw), ctypes.c_longlong(len(raw)), L.i32(S), ctypes.c_void_p(out.ctypes.data),
                                    ctypes.c_longlong(out.size)))
    if n == -10:
        raise ValueError(f"build_index: file not indexed ({INDEX_REASONS[int(out[:4].view('<i4')[0])]})")
    if n <= 0:
        raise ValueError(f"build_index: {ERRORS.get(n, 'error')} (code {n})")
    return out[:n].tobytes()


def index_info(index):
    """The fields of an index's header.  ``ValueError`` for bytes that are not an index of this version."""
    index = _as_bytes(index)
    if len(index) < INDEX_HEAD_BYTES + 16:
        raise ValueError("index_info: too short for an index")
    w = np.frombuffer(index, "<u4", 32)
    if int(w[0]) != INDEX_MAGIC or int(w[1]) != INDEX_VERSION:
        raise ValueError(f"index_info: magic {int(w[0]):#x} version {int(w[1])}: not an index of version {INDEX_VERSION}")
    return JpegIndexInfo(int(w[2]) | int(w[3]) << 32, int(w[4]) | int(w[5]) << 32, int(w[6]), int(w[7]), int(w[8]), int(w[9]),
                         int(w[10]), int(w[11]), int(w[12]), int(w[13]), int(w[14]), int(w[16]) | int(w[17]) << 32)


def index_stage(raw, index, window=None, verify=False):
    """The host half of the indexed path on its own (no GPU): ``(record, stream_record, pool)`` -- the dense record, the
    stream record and the uint8 bytes ``fv_jpeg_index_stage`` appends to a stream pool for the MCU ``window`` (default: the
    whole image; the record's offsets count from 0).  ``ValueError`` with the reason where the index does not fit the file."""
    raw, index = _as_bytes(raw), _as_bytes(index)
    ix = index_info(index)
    win = (0, 0, ix.mcus_x, ix.mcus_y) if window is None else tuple(int(v) for v in window)
    pool = _aligned_bytes(len(raw) + len(index) + 64)
    rec, srec, used = np.zeros(REC_INTS, np.int32), np.zeros(SREC_INTS, np.int32), ctypes.c_longlong(0)
    rc = L.host_lib().fv_jpeg_index_stage(ctypes.c_char_p(raw), ctypes.c_longlong(len(raw)), ctypes.c_char_p(index),
                                          ctypes.c_longlong(len(index)), (ctypes.c_int * 4)(*win), L.i32(bool(verify)),
                                          ctypes.c_void_p(pool.ctypes.data), ctypes.c_longlong(pool.size), ctypes.byref(used),
                                          ctypes.c_longlong(0), ctypes.c_void_p(rec.ctypes.data), ctypes.c_void_p(srec.ctypes.data))
    if rc != 0:
        raise ValueError(f"fv_jpeg_index_stage: {INDEX_ERRORS.get(rc, ERRORS.get(rc, 'error'))} (code {rc})")
    return rec, srec, pool[:used.value].copy()


def sync_stage(raw, window=None, segment_mcus=DEFAULT_SEGMENT_MCUS, subseq_bytes=DEFAULT_SUBSEQ_BYTES, max_scan_bytes=1 << 20,
               pool_capacity_bytes=None, run=True):
    """The index-free path on the host alone (no GPU): ``fv_jpeg_sync_stage`` of the MCU ``window`` (default: the whole
    image) into a fresh stream pool, then -- with ``run`` -- ``fv_jpeg_sync_host``, the passes of ``fv_jpeg_sync`` run serially
    on the CPU.  Returns ``(record, stream_record, job, pool)``; the entries are ``pool[job[17]:][:16 * groups]``, the
    status and the rounds ``job[24]`` and ``job[25]``.  ``ValueError`` with the code for a file or a capacity the stage
    function refuses (``.args[1]`` is the code, ``.args[2]`` the FV_JPEG_R_* reason of an unserved file)."""
    raw = _as_bytes(raw)
    info = _probe(raw)
    win = (0, 0, max(info[6], 1), max(info[7], 1)) if window is None else tuple(int(v) for v in window)
    cap = len(raw) + 8192 + 16 * max(win[2] * win[3], 0) if pool_capacity_bytes is None else int(pool_capacity_bytes)
    pool = _aligned_bytes(max(cap, 16))
    before = pool.copy()
    records = len(raw) // int(subseq_bytes) + 2 if int(subseq_bytes) > 0 else 2
    scratch = np.zeros(records * SYNC_REC_BYTES // 4, np.uint32)
    rec, srec, job = np.zeros(REC_INTS, np.int32), np.zeros(SREC_INTS, np.int32), np.zeros(SYNC_JOB_INTS, np.int32)
    used, rused = ctypes.c_longlong(0), ctypes.c_longlong(0)
    lib = L.host_lib()
    rc = lib.fv_jpeg_sync_stage(ctypes.c_char_p(raw), ctypes.c_longlong(len(raw)), (ctypes.c_int * 4)(*win), L.i32(segment_mcus),
                                L.i32(subseq_bytes), ctypes.c_longlong(int(max_scan_bytes)), ctypes.c_void_p(pool.ctypes.data),
                                ctypes.c_longlong(cap), ctypes.byref(used), ctypes.c_longlong(records), ctypes.byref(rused),
                                ctypes.c_longlong(0), ctypes.c_void_p(rec.ctypes.data), ctypes.c_void_p(srec.ctypes.data),
                                ctypes.c_void_p(job.ctypes.data))
    if rc != 0:
        assert np.array_equal(pool, before) and used.value == 0 and rused.value == 0      # a refusal leaves the pool and both counters alone (an unserved file: job[0] = 0, job[1] = the reason)
        raise ValueError(f"fv_jpeg_sync_stage: code {rc}", rc, int(job[1]))
    if run:
        rc = lib.fv_jpeg_sync_host(ctypes.c_void_p(pool.ctypes.data), ctypes.c_longlong(used.value), ctypes.c_void_p(job.ctypes.data),
                                   ctypes.c_void_p(scratch.ctypes.data), ctypes.c_longlong(records))
        if rc != 0:
            raise ValueError(f"fv_jpeg_sync_host: code {rc}", rc, 0)
    return rec, srec, job, pool[:used.value].copy()


def _pil_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


class JpegImageStage(ImageStage):
    """An ``ImageStage`` whose samples may also be put as JPEG FILES.  Each ring slot gains a pinned and a device pool of
    int16 coefficients (``coef_capacity_bytes``) and the table of sample records; the plane workspace between the two JPEG
    launches is shared by the slots like the resampler's coefficient workspace (launches of one stream are ordered).

    ``put`` and ``put_jpeg`` may be mixed within a batch; a sample put as a decoded array has a zero-length JPEG job.
    ``commit()`` also copies the used part of the coefficient pool and the table; ``resample(out)`` runs ``fv_jpeg_idct``
    and ``fv_jpeg_rgb`` (``decode()``) in front of the two resample launches.  Their grids depend on the capacities only,
    so with ``slots=1`` a captured ``resample`` replays correctly after a ``commit()`` of any other batch.

    ``coef_format="packed"`` (default ``"dense"``) stages the packed form: ``coef_capacity_bytes`` then bounds the packed
    pool of a slot, and ``plane_capacity_bytes`` the plane workspace, 64 bytes per block, which the packed pool no longer
    implies (default ``4 * coef_capacity_bytes``: enough while a block packs to 16 bytes or more, and a header alone is
    16).  A sample's packed size is known only after it is decoded: ``put_jpeg`` decodes into a scratch buffer of the
    calling thread, reserves the exact size under the lock and copies into the pinned pool outside it, so the pool's
    layout follows the order in which threads finish -- the pixels do not.  ``decode()`` runs ``fv_jpeg_idct_packed``.

    ``stream_capacity_bytes`` (default 0: none of this exists) sets up the INDEXED path of the dense form: per slot a pinned
    and a device STREAM POOL -- per indexed sample the four Huffman tables, the index entries of the groups its MCU window
    meets and the file bytes of those groups -- the stream table and its status words.  ``put_jpeg_indexed`` fills them;
    its coefficients never cross the link: their space is taken from the TOP of the coefficient pool downward, against
    the same ``coef_capacity_bytes``, and ``fv_jpeg_huff`` writes them in front of ``fv_jpeg_idct``.  ``segment_capacity``
    bounds the groups (lanes) of a batch; 0: only the stream pool bounds them, 16 bytes each.

    ``sync=True`` (default False: none of this exists; needs ``stream_capacity_bytes``) adds the INDEX-FREE path:
    ``put_jpeg_sync`` stages the tables, a reserved entry region and the WHOLE SCAN of a file (at most ``max_scan_bytes``) in
    the stream pool, with groups of ``segment_mcus`` MCUs, and a sync job; ``fv_jpeg_sync`` runs in front of
    ``fv_jpeg_huff`` and writes the entries, working on subsequences of ``subseq_bytes`` (a power of two in [16, 1024];
    default ``DEFAULT_SUBSEQ_BYTES``) whose states live in a scratch buffer the slots share, 32 bytes per subsequence the
    stream pool can hold."""

    def __init__(self, batch, out_size, capacity_bytes, coef_capacity_bytes, slots=2, device=None, coef_format="dense",
                 plane_capacity_bytes=None, stream_capacity_bytes=0, segment_capacity=0, sync=False, subseq_bytes=None,
                 max_scan_bytes=1 << 20, segment_mcus=DEFAULT_SEGMENT_MCUS):
        if coef_format not in ("dense", "packed"):
            raise ValueError(f"JpegImageStage: coef_format {coef_format!r} is neither 'dense' nor 'packed'")
        if int(stream_capacity_bytes) < 0 or int(segment_capacity) < 0:
            raise ValueError("JpegImageStage: negative stream_capacity_bytes or segment_capacity")
        if int(stream_capacity_bytes) and coef_format != "dense":
            raise ValueError("JpegImageStage: the indexed path (stream_capacity_bytes) writes dense coefficients: "
                             "coef_format='packed' is not accepted with it")
        if int(segment_capacity) and not int(stream_capacity_bytes):
            raise ValueError("JpegImageStage: segment_capacity belongs to the indexed path (stream_capacity_bytes)")
        self.sync = bool(sync)
        if self.sync:
            if coef_format != "dense":
                raise ValueError("JpegImageStage: sync=True writes dense coefficients through fv_jpeg_huff: "
                                 "coef_format='packed' is not accepted with it")
            if not int(stream_capacity_bytes):
                raise ValueError("JpegImageStage: sync=True needs stream_capacity_bytes (the scans are staged in the stream pool)")
            self.subseq_bytes = DEFAULT_SUBSEQ_BYTES if subseq_bytes is None else int(subseq_bytes)
            if not 16 <= self.subseq_bytes <= 1024 or self.subseq_bytes & (self.subseq_bytes - 1):
                raise ValueError(f"JpegImageStage: subseq_bytes {self.subseq_bytes} is not a power of two in [16, 1024]")
            self.max_scan_bytes, self.segment_mcus = int(max_scan_bytes), int(segment_mcus)
            if self.max_scan_bytes < 1 or not 1 <= self.segment_mcus <= 65536:
                raise ValueError("JpegImageStage: max_scan_bytes below 1 or segment_mcus outside [1, 65536]")
            # a job has at most SYNC_MAX_SUBSEQS subsequences (the rounds of a launch are bounded by them): a longer scan is
            # refused by the stage function like one above max_scan_bytes, and takes the put_jpeg route
            self.max_scan_bytes = min(self.max_scan_bytes, SYNC_MAX_SUBSEQS * self.subseq_bytes)
        elif subseq_bytes is not None or int(max_scan_bytes) != 1 << 20 or int(segment_mcus) != DEFAULT_SEGMENT_MCUS:
            raise ValueError("JpegImageStage: subseq_bytes, max_scan_bytes and segment_mcus belong to sync=True")
        super().__init__(batch, out_size, capacity_bytes, slots=slots, device=device)
        self.coef_format = coef_format
        self._lock = threading.RLock()
        self.last_jpeg_fallbacks = 0
        self.staged_coef_bytes = 0             # coefficient bytes of the batch committed last (packed: the pool bytes used)
        self.staged_pool_bytes = 0             # of ``staged_bytes`` (pool bytes in use), those the host filled and sent
        self.stream_bytes = (int(stream_capacity_bytes) + 15) // 16 * 16
        self.segment_capacity = int(segment_capacity)
        self.staged_stream_bytes = 0           # stream pool bytes of the batch committed last: tables, entries, file bytes
        self.last_sync_fallbacks = 0           # of the batch committed last: files put_jpeg_sync sent the put_jpeg route
        n = int(L.lib().fv_jpeg_table_ints(L.i32(self.batch)))
        assert n == self.batch * REC_INTS + 2 * (self.batch + 1)
        for s in self._slots:
            s.table_pin = torch.zeros(n, dtype=torch.int32).pin_memory()
            s.table_np = s.table_pin.numpy()
            s.records = s.table_np[:self.batch * REC_INTS].reshape(self.batch, REC_INTS)
            s.table = torch.zeros(n, dtype=torch.int32, device=self.device)
            s.jused, s.pused, s.jfallbacks = 0, 0, 0
            s.jtop, s.sused, s.lanes = 0, 0, 0
        if coef_format == "packed":
            self.coef_bytes = (int(coef_capacity_bytes) + 15) // 16 * 16
            planes = 4 * self.coef_bytes if plane_capacity_bytes is None else int(plane_capacity_bytes)
            self.plane_bytes = (planes + 63) // 64 * 64
            for s in self._slots:
                s.coef_pin = torch.zeros(self.coef_bytes, dtype=torch.uint8).pin_memory()
                s.coef = torch.zeros(self.coef_bytes, dtype=torch.uint8, device=self.device)
            self._planes = torch.zeros(self.plane_bytes, dtype=torch.uint8, device=self.device)
            self._scratch = threading.local()
            return
        if plane_capacity_bytes is not None:
            raise ValueError("JpegImageStage: plane_capacity_bytes belongs to coef_format='packed' (the dense form's plane "
                             "workspace has the size of its coefficient pool)")
        self.coef_elems = (int(coef_capacity_bytes) + 127) // 128 * 64
        for s in self._slots:
            s.coef_pin = torch.zeros(self.coef_elems, dtype=torch.int16).pin_memory()
            s.coef = torch.zeros(self.coef_elems, dtype=torch.int16, device=self.device)
        self._planes = torch.zeros(self.coef_elems, dtype=torch.uint8, device=self.device)
        if self.stream_bytes:
            m = int(L.lib().fv_jpeg_stream_table_ints(L.i32(self.batch)))
            assert m == self.batch * SREC_INTS + self.batch + 1
            for s in self._slots:
                s.stream_pin = torch.zeros(self.stream_bytes, dtype=torch.uint8).pin_memory()
                s.stream = torch.zeros(self.stream_bytes + 16, dtype=torch.uint8, device=self.device)      # a zero tail
                s.stable_pin = torch.zeros(m, dtype=torch.int32).pin_memory()
                s.stable_np = s.stable_pin.numpy()
                s.srecords = s.stable_np[:self.batch * SREC_INTS].reshape(self.batch, SREC_INTS)
                s.stable = torch.zeros(m, dtype=torch.int32, device=self.device)
        if self.sync:
            m = int(L.lib().fv_jpeg_sync_table_ints(L.i32(self.batch)))
            assert m == self.batch * SYNC_JOB_INTS
            self.sync_records = self.stream_bytes // self.subseq_bytes + self.batch      # a scan's last subsequence may be short
            self._sync_scratch = torch.zeros(self.sync_records * SYNC_REC_BYTES // 4, dtype=torch.int32, device=self.device)
            for s in self._slots:
                s.sync_pin = torch.zeros(m, dtype=torch.int32).pin_memory()
                s.sjobs = s.sync_pin.numpy().reshape(self.batch, SYNC_JOB_INTS)
                s.sync = torch.zeros(m, dtype=torch.int32, device=self.device)
                s.rused, s.sfallbacks = 0, 0

    def _filling(self):
        fresh = not self._open
        s = super()._filling()
        if fresh:
            s.records[:, 0] = 0                # no JPEG job anywhere
            s.jused, s.pused, s.jfallbacks = 0, 0, 0
            s.jtop, s.sused, s.lanes = getattr(self, "coef_elems", 0), 0, 0      # indexed samples reserve from the top down
            if self.stream_bytes:
                s.srecords[:] = 0
            if self.sync:
                s.sjobs[:] = 0
                s.rused, s.sfallbacks = 0, 0
        return s

    def put(self, i, array_hwc_u8, crop=None, out_full=None, window=(0, 0), flip=False):
        with self._lock:
            super().put(i, array_hwc_u8, crop=crop, out_full=out_full, window=window, flip=flip)

    def _put_decoded(self, i, data, crop, out_full, window, flip):
        try:
            a = _pil_decode(data)
        except ImportError:
            raise ValueError(f"JpegImageStage.put_jpeg: sample {i} is outside the device path and PIL is not importable "
                             "for the host fallback") from None
        with self._lock:
            self.put(i, a, crop=crop, out_full=out_full, window=window, flip=flip)
            self._slots[self._fill].jfallbacks += 1

    def put_jpeg(self, i, data, crop=None, out_full=None, window=(0, 0), flip=False):
        """Stage sample ``i`` from the bytes of a JPEG file: the same meaning as ``put`` of the decoded image.  Reserves the
        crop's region of the pixel pool, writes the ordinary plan row and entropy-decodes the MCUs the crop needs into the
        pinned coefficient pool.  The decode is one ctypes call, and ctypes releases the GIL for its length: loader
        threads that call ``put_jpeg`` for different samples decode in parallel (the reservations are under a lock).
        With ``coef_format="packed"`` the decode comes first, into a scratch buffer of the thread, and the reservation of the
        exact packed size after it (``_put_packed``)."""
        i, data = int(i), _as_bytes(data)
        H, W, _, cls, ok, _, _, _ = _probe(data)
        if not ok:
            return self._put_decoded(i, data, crop, out_full, window, flip)
        t, l, h, w = (0, 0, H, W) if crop is None else (int(v) for v in crop)
        if min(t, l) < 0 or h < 1 or w < 1 or t + h > H or l + w > W:
            raise ValueError(f"ImageStage.put: crop {tuple(crop)} of sample {i} does not lie inside its {H}x{W} image")
        o_h, o_w = (self.s_h, self.s_w) if out_full is None else _pair(out_full)
        win_y, win_x = (int(v) for v in window)
        if o_h < 1 or o_w < 1 or win_y < 0 or win_x < 0 or win_y + self.s_h > o_h or win_x + self.s_w > o_w:
            raise ValueError(f"ImageStage.put: the {self.s_h}x{self.s_w} window at {(win_y, win_x)} of sample {i} does not lie "
                             f"inside its {o_h}x{o_w} resize")
        if not resample_ok(self.batch, self.s_h, self.s_w, h, w, o_h, o_w, win_y, win_x):
            return self._put_decoded(i, data, crop, out_full, window, flip)      # ``put`` resizes it with PIL on the host
        mcus = mcu_window(H, W, cls, (t, l, h, w))
        n = window_elements(cls, mcus)
        if self.coef_format == "packed":
            return self._put_packed(i, data, cls, mcus, n // 64, (t, l, h, w), (o_h, o_w), (win_y, win_x), flip)
        with self._lock:
            s = self._filling()
            if not 0 <= i < self.batch:
                raise IndexError(f"ImageStage.put: sample {i} of a batch of {self.batch}")
            if s.host.filled[i]:
                raise ValueError(f"ImageStage.put: sample {i} was already put in this batch")
            if s.jused + n > s.jtop:           # the capacity, less what indexed samples of the batch took from the top
                raise ValueError(f"JpegImageStage.put_jpeg: sample {i} ({2 * n} coefficient bytes at offset {2 * s.jused}) "
                                 f"overflows coef_capacity_bytes = {2 * self.coef_elems}")
            off = s.host.reserve(i, h, w, o_h, o_w, win_y, win_x, flip)
            base, s.jused = s.jused, s.jused + n
        rec = s.records[i]
        rc = L.host_lib().fv_jpeg_entropy_decode(ctypes.c_char_p(data), ctypes.c_longlong(len(data)), (ctypes.c_int * 4)(*mcus),
                                                 ctypes.c_void_p(s.coef_pin.data_ptr() + 2 * base), ctypes.c_longlong(n),
                                                 ctypes.c_void_p(rec.ctypes.data))
        if rc != 0:
            # a file the decoder gives up on: PIL's pixels into the region already reserved (PIL's own exception propagates
            # for a file it rejects too)
            rec[:] = 0
            try:
                a = _pil_decode(data)
            except ImportError:
                raise ValueError(f"JpegImageStage.put_jpeg: sample {i}: {ERRORS.get(rc, 'error')} (code {rc}), and PIL is not "
                                 "importable for the host fallback") from None
            np.copyto(s.host.pool[off:off + h * w * 3].reshape(h, w, 3), a[t:t + h, l:l + w])
            with self._lock:
                s.jfallbacks += 1
            return
        u = rec.view(np.uint32)
        for c in range(1 if cls == GRAY else 3):                   # offsets relative to the sample -> to the pool
            e = (int(u[9 + 2 * c]) | int(u[10 + 2 * c]) << 32) + base
            u[9 + 2 * c], u[10 + 2 * c] = e & 0xffffffff, e >> 32
        rec[19:23] = (t, l, h, w)
        u[23], u[24] = off & 0xffffffff, off >> 32

    def put_jpeg_indexed(self, i, data, index, crop=None, out_full=None, window=(0, 0), flip=False, verify=False):
        """``put_jpeg`` of a file whose index (``build_index``) is at hand: the same meaning, argument checks and PIL
        fallback outside the resampler's range -- but no Huffman code is decoded here.  The index is checked against the
        file (magic, version, size; with ``verify`` the hash of the bytes too; every entry used inside the scan and in
        file order: ``ValueError`` otherwise), then the tables, the entries of the groups the crop's MCU window meets and the
        file bytes of those groups are copied into the pinned stream pool (one foreign call), and the ordinary dense
        record and the stream record are written.  The window's coefficient space is reserved from the top of the
        coefficient pool; ``fv_jpeg_huff`` fills it on the device."""
        if not self.stream_bytes:
            raise RuntimeError("JpegImageStage.put_jpeg_indexed: the stage was built without stream_capacity_bytes")
        i, data, index = int(i), _as_bytes(data), _as_bytes(index)
        try:
            ix = index_info(index)
        except ValueError as e:
            raise ValueError(f"JpegImageStage.put_jpeg_indexed: sample {i}: {e}") from None
        if ix.nbytes != len(data):
            raise ValueError(f"JpegImageStage.put_jpeg_indexed: sample {i}: the index is of a file of {ix.nbytes} bytes, not {len(data)}")
        H, W, cls = ix.height, ix.width, ix.subsampling
        if not (0 <= cls <= 3 and 1 <= H <= 65535 and 1 <= W <= 65535 and 1 <= ix.segment_mcus <= 65536):
            raise ValueError(f"JpegImageStage.put_jpeg_indexed: sample {i}: {INDEX_ERRORS[-17]}")
        t, l, h, w = (0, 0, H, W) if crop is None else (int(v) for v in crop)
        if min(t, l) < 0 or h < 1 or w < 1 or t + h > H or l + w > W:
            raise ValueError(f"ImageStage.put: crop {tuple(crop)} of sample {i} does not lie inside its {H}x{W} image")
        o_h, o_w = (self.s_h, self.s_w) if out_full is None else _pair(out_full)
        win_y, win_x = (int(v) for v in window)
        if o_h < 1 or o_w < 1 or win_y < 0 or win_x < 0 or win_y + self.s_h > o_h or win_x + self.s_w > o_w:
            raise ValueError(f"ImageStage.put: the {self.s_h}x{self.s_w} window at {(win_y, win_x)} of sample {i} does not lie "
                             f"inside its {o_h}x{o_w} resize")
        if not resample_ok(self.batch, self.s_h, self.s_w, h, w, o_h, o_w, win_y, win_x):
            return self._put_decoded(i, data, crop, out_full, window, flip)      # ``put`` resizes it with PIL on the host
        mcus = mcu_window(H, W, cls, (t, l, h, w))
        n = window_elements(cls, mcus)
        S = ix.segment_mcus
        lanes = ((mcus[0] + mcus[2] - 1) // S - mcus[0] // S + 1) * mcus[3]
        with self._lock:
            s = self._filling()
            if not 0 <= i < self.batch:
                raise IndexError(f"ImageStage.put: sample {i} of a batch of {self.batch}")
            if s.host.filled[i]:
                raise ValueError(f"ImageStage.put: sample {i} was already put in this batch")
            if s.jtop - n < s.jused:
                raise ValueError(f"JpegImageStage.put_jpeg_indexed: sample {i} ({2 * n} coefficient bytes below offset {2 * s.jtop}) "
                                 f"overflows coef_capacity_bytes = {2 * self.coef_elems}")
            if self.segment_capacity and s.lanes + lanes > self.segment_capacity:
                raise ValueError(f"JpegImageStage.put_jpeg_indexed: sample {i} ({lanes} groups after {s.lanes}) overflows "
                                 f"segment_capacity = {self.segment_capacity}")
            at = (s.host.used + ALIGN - 1) // ALIGN * ALIGN            # ``reserve``'s own check, before anything is written
            if at + h * w * 3 > self.capacity:
                raise ValueError(f"ImageStage.put: sample {i} ({h * w * 3} bytes at offset {at}) overflows capacity_bytes = "
                                 f"{self.capacity}")
            rec, srec, used = s.records[i], s.srecords[i], ctypes.c_longlong(s.sused)
            rc = L.host_lib().fv_jpeg_index_stage(ctypes.c_char_p(data), ctypes.c_longlong(len(data)), ctypes.c_char_p(index),
                                                  ctypes.c_longlong(len(index)), (ctypes.c_int * 4)(*mcus), L.i32(bool(verify)),
                                                  ctypes.c_void_p(s.stream_pin.data_ptr()), ctypes.c_longlong(self.stream_bytes),
                                                  ctypes.byref(used), ctypes.c_longlong(s.jtop - n),
                                                  ctypes.c_void_p(rec.ctypes.data), ctypes.c_void_p(srec.ctypes.data))
            if rc != 0:
                rec[:] = 0
                srec[:] = 0
                what = "stream_capacity_bytes" if rc == -15 else "the index"
                raise ValueError(f"JpegImageStage.put_jpeg_indexed: sample {i}: {INDEX_ERRORS.get(rc, ERRORS.get(rc, 'error'))} "
                                 f"(code {rc}; {what})")
            off = s.host.reserve(i, h, w, o_h, o_w, win_y, win_x, flip)
            s.jtop, s.sused, s.lanes = s.jtop - n, used.value, s.lanes + lanes
            rec[19:23] = (t, l, h, w)
            rec.view(np.uint32)[23:25] = (off & 0xffffffff, off >> 32)

    def put_jpeg_sync(self, i, data, crop=None, out_full=None, window=(0, 0), flip=False):
        """``put_jpeg_indexed`` of a file WITHOUT an index: the same meaning, argument checks and PIL fallback outside the
        resampler's range, and no Huffman code is decoded here.  The markers are parsed, and the tables, a reserved entry
        region for the groups the crop's MCU window meets and the whole scan are copied into the pinned stream pool (one
        foreign call) with the dense record, the stream record and the sync job; ``fv_jpeg_sync`` writes the entries on
        the device and ``fv_jpeg_huff`` the coefficients.  A file the stage function refuses -- unserved, a restart
        interval, separate chroma tables, fill bytes inside the scan, a scan above ``max_scan_bytes`` -- goes through
        ``put_jpeg`` inside this call and is counted in ``last_sync_fallbacks``: one call for any ``.jpg``.

        NOT caught here: a file whose markers parse but whose scan is damaged or cut short (a stray RSTn without a restart
        interval, missing bytes).  ``put_jpeg`` decodes on the host and would fall back to PIL or raise for it; this call
        decodes nothing, so the damage shows only on the device: ``fv_jpeg_sync`` gives the sample status 6 and writes no
        entry, its coefficients and pixels in the batch are unspecified, and nothing raises -- ``stream_status()``, which
        synchronises, is the only place it is visible.  A loader that cannot vouch for its files checks ``stream_status()``
        per batch or keeps ``put_jpeg`` for them."""
        if not self.sync:
            raise RuntimeError("JpegImageStage.put_jpeg_sync: the stage was built without sync=True")
        i, data = int(i), _as_bytes(data)
        H, W, _, cls, ok, _, _, _ = _probe(data)
        if not ok:
            return self._put_sync_refused(i, data, crop, out_full, window, flip)
        t, l, h, w = (0, 0, H, W) if crop is None else (int(v) for v in crop)
        if min(t, l) < 0 or h < 1 or w < 1 or t + h > H or l + w > W:
            raise ValueError(f"ImageStage.put: crop {tuple(crop)} of sample {i} does not lie inside its {H}x{W} image")
        o_h, o_w = (self.s_h, self.s_w) if out_full is None else _pair(out_full)
        win_y, win_x = (int(v) for v in window)
        if o_h < 1 or o_w < 1 or win_y < 0 or win_x < 0 or win_y + self.s_h > o_h or win_x + self.s_w > o_w:
            raise ValueError(f"ImageStage.put: the {self.s_h}x{self.s_w} window at {(win_y, win_x)} of sample {i} does not lie "
                             f"inside its {o_h}x{o_w} resize")
        if not resample_ok(self.batch, self.s_h, self.s_w, h, w, o_h, o_w, win_y, win_x):
            return self._put_decoded(i, data, crop, out_full, window, flip)      # ``put`` resizes it with PIL on the host
        mcus = mcu_window(H, W, cls, (t, l, h, w))
        n = window_elements(cls, mcus)
        S = self.segment_mcus
        lanes = ((mcus[0] + mcus[2] - 1) // S - mcus[0] // S + 1) * mcus[3]
        with self._lock:
            s = self._filling()
            if not 0 <= i < self.batch:
                raise IndexError(f"ImageStage.put: sample {i} of a batch of {self.batch}")
            if s.host.filled[i]:
                raise ValueError(f"ImageStage.put: sample {i} was already put in this batch")
            if s.jtop - n < s.jused:
                raise ValueError(f"JpegImageStage.put_jpeg_sync: sample {i} ({2 * n} coefficient bytes below offset {2 * s.jtop}) "
                                 f"overflows coef_capacity_bytes = {2 * self.coef_elems}")
            if self.segment_capacity and s.lanes + lanes > self.segment_capacity:
                raise ValueError(f"JpegImageStage.put_jpeg_sync: sample {i} ({lanes} groups after {s.lanes}) overflows "
                                 f"segment_capacity = {self.segment_capacity}")
            at = (s.host.used + ALIGN - 1) // ALIGN * ALIGN            # ``reserve``'s own check, before anything is written
            if at + h * w * 3 > self.capacity:
                raise ValueError(f"ImageStage.put: sample {i} ({h * w * 3} bytes at offset {at}) overflows capacity_bytes = "
                                 f"{self.capacity}")
            rec, srec, job = s.records[i], s.srecords[i], s.sjobs[i]
            used, rused = ctypes.c_longlong(s.sused), ctypes.c_longlong(s.rused)
            rc = L.host_lib().fv_jpeg_sync_stage(ctypes.c_char_p(data), ctypes.c_longlong(len(data)), (ctypes.c_int * 4)(*mcus),
                                                 L.i32(S), L.i32(self.subseq_bytes), ctypes.c_longlong(self.max_scan_bytes),
                                                 ctypes.c_void_p(s.stream_pin.data_ptr()), ctypes.c_longlong(self.stream_bytes),
                                                 ctypes.byref(used), ctypes.c_longlong(self.sync_records), ctypes.byref(rused),
                                                 ctypes.c_longlong(s.jtop - n), ctypes.c_void_p(rec.ctypes.data),
                                                 ctypes.c_void_p(srec.ctypes.data), ctypes.c_void_p(job.ctypes.data))
            if rc == 0:
                off = s.host.reserve(i, h, w, o_h, o_w, win_y, win_x, flip)
                s.jtop, s.sused, s.rused, s.lanes = s.jtop - n, used.value, rused.value, s.lanes + lanes
                rec[19:23] = (t, l, h, w)
                rec.view(np.uint32)[23:25] = (off & 0xffffffff, off >> 32)
                return
            rec[:] = 0
            srec[:] = 0
            job[:] = 0
            if rc not in SYNC_REFUSALS:
                what = "stream_capacity_bytes" if rc == -15 else "the file"
                raise ValueError(f"JpegImageStage.put_jpeg_sync: sample {i}: {INDEX_ERRORS.get(rc, ERRORS.get(rc, 'error'))} "
                                 f"(code {rc}; {what})")
        return self._put_sync_refused(i, data, crop, out_full, window, flip)

    def _put_sync_refused(self, i, data, crop, out_full, window, flip):
        with self._lock:
            self.put_jpeg(i, data, crop=crop, out_full=out_full, window=window, flip=flip)
            self._slots[self._fill].sfallbacks += 1

    def _put_packed(self, i, data, cls, mcus, blocks, crop, out_full, window, flip):
        """``put_jpeg`` of the packed form: decode into this thread's scratch, reserve the exact size, copy."""
        bound = 142 * blocks                                           # fv_jpeg_packed_bound
        tl = self._scratch
        if getattr(tl, "size", -1) < bound:
            tl.buf = _aligned_bytes(max(bound, 1 << 16))
            tl.size, tl.ptr = tl.buf.size, ctypes.c_void_p(tl.buf.ctypes.data)
            tl.rec = np.zeros(REC_INTS, np.int32)
            tl.rec_ptr = ctypes.c_void_p(tl.rec.ctypes.data)
        rec = tl.rec
        rc = L.host_lib().fv_jpeg_entropy_decode_packed(ctypes.c_char_p(data), ctypes.c_longlong(len(data)), (ctypes.c_int * 4)(*mcus),
                                                        tl.ptr, ctypes.c_longlong(bound), tl.rec_ptr)
        if rc != 0:
            return self._put_decoded(i, data, crop, out_full, window, flip)      # a file the decoder gives up on
        t, l, h, w = crop
        nbytes, planes = _rec_i64(rec, 15), 64 * blocks
        with self._lock:
            s = self._filling()
            if not 0 <= i < self.batch:
                raise IndexError(f"ImageStage.put: sample {i} of a batch of {self.batch}")
            if s.host.filled[i]:
                raise ValueError(f"ImageStage.put: sample {i} was already put in this batch")
            if s.jused + nbytes > self.coef_bytes:
                raise ValueError(f"JpegImageStage.put_jpeg: sample {i} ({nbytes} packed coefficient bytes at offset {s.jused}) "
                                 f"overflows coef_capacity_bytes = {self.coef_bytes}")
            if s.pused + planes > self.plane_bytes:
                raise ValueError(f"JpegImageStage.put_jpeg: sample {i} ({planes} plane bytes at offset {s.pused}) overflows "
                                 f"plane_capacity_bytes = {self.plane_bytes}")
            off = s.host.reserve(i, h, w, out_full[0], out_full[1], window[0], window[1], flip)
            base, pbase = s.jused, s.pused
            s.jused, s.pused = (base + nbytes + 15) // 16 * 16, pbase + planes
        ctypes.memmove(s.coef_pin.data_ptr() + base, tl.ptr, nbytes)       # a foreign call: the GIL is released
        for c in range(1 if cls == GRAY else 3):                   # offsets relative to the sample -> to the workspaces
            _rec_add(rec, 9 + 2 * c, pbase)
        _rec_add(rec, 25, base)
        _rec_add(rec, 27, base)
        rec[19:23] = crop
        rec.view(np.uint32)[23:25] = (off & 0xffffffff, off >> 32)
        s.records[i] = rec

    def _copy_pool(self, s):
        """Only the regions the HOST filled cross the link (samples put as arrays, fallbacks); a JPEG job's region is
        written by ``fv_jpeg_rgb``.  Neighbouring host regions go as one copy -- what lies between them is overwritten by
        the launches anyway."""
        host = np.flatnonzero(s.records[:, 0] == 0)
        spans = sorted((s.host.offset(i), int(s.host.plan[i, 2]) * int(s.host.plan[i, 3]) * 3) for i in host)
        runs = []
        for off, n in spans:
            if runs and off - runs[-1][1] <= 4096:
                runs[-1][1] = off + n
            else:
                runs.append([off, off + n])
        for lo, hi in runs:
            s.pool[lo:hi].copy_(s.pool_pin[lo:hi], non_blocking=True)
        self.staged_pool_bytes = sum(n for _, n in spans)

    def commit(self):
        with self._lock:
            s = self._filling()
            s.host.check_complete()
            r = s.records
            job = r[:, 0] != 0
            blocks = np.where(job, r[:, 17], 0).astype(np.int64)
            quads = np.where(job, (r[:, 21].astype(np.int64) * r[:, 22] + 3) // 4, 0)
            pre = np.zeros((2, self.batch + 1), np.int64)
            np.cumsum(blocks, out=pre[0, 1:])
            np.cumsum(quads, out=pre[1, 1:])
            if pre.max() > 0x7fffffff:
                raise ValueError("JpegImageStage.commit: more than 2^31 - 1 blocks or pixel quads in one batch")
            s.table_np[self.batch * REC_INTS:] = pre.reshape(-1)
            s.coef[:s.jused].copy_(s.coef_pin[:s.jused], non_blocking=True)
            s.table.copy_(s.table_pin, non_blocking=True)
            if self.stream_bytes:
                sr = s.srecords
                lanes = np.where(sr[:, 0] == 1, sr[:, 9].astype(np.int64) * sr[:, 5], 0)
                np.cumsum(lanes, out=pre[0, 1:])
                if pre[0].max() > 0x7fffffff:
                    raise ValueError("JpegImageStage.commit: more than 2^31 - 1 groups in one batch")
                s.stable_np[self.batch * SREC_INTS:] = pre[0]
                s.stream[:s.sused].copy_(s.stream_pin[:s.sused], non_blocking=True)
                s.stable.copy_(s.stable_pin, non_blocking=True)
                self.staged_stream_bytes = s.sused
            if self.sync:
                s.sync.copy_(s.sync_pin, non_blocking=True)
                self.last_sync_fallbacks = s.sfallbacks
            self.last_jpeg_fallbacks = s.jfallbacks
            self.staged_coef_bytes = s.jused if self.coef_format == "packed" else 2 * s.jused
            super().commit()

    def decode(self):
        """The two JPEG launches on the slot committed last: coefficients -> sample planes (``fv_jpeg_idct``, or
        ``fv_jpeg_idct_packed`` on the packed form), planes -> RGB crops in the pixel pool (``fv_jpeg_rgb``)."""
        s = self._ready
        if s is None:
            raise RuntimeError("JpegImageStage.decode: nothing was committed")
        lib, st, b = L.lib(), L.stream_of(s.pool), L.i32(self.batch)
        if self.coef_format == "packed":
            ne = ctypes.c_longlong(self.plane_bytes)
            L.check(lib.fv_jpeg_idct_packed(L.ptr(s.coef), ctypes.c_longlong(self.coef_bytes), L.ptr(s.table), L.ptr(self._planes),
                                            ne, b, st), "fv_jpeg_idct_packed")
        else:
            ne = ctypes.c_longlong(self.coef_elems)
            if self.sync:
                L.check(lib.fv_jpeg_sync(L.ptr(s.stream), ctypes.c_longlong(self.stream_bytes), L.ptr(s.sync), L.ptr(self._sync_scratch),
                                         ctypes.c_longlong(self.sync_records * SYNC_REC_BYTES), b, st), "fv_jpeg_sync")
            if self.stream_bytes:
                L.check(lib.fv_jpeg_huff(L.ptr(s.stream), ctypes.c_longlong(self.stream_bytes), L.ptr(s.stable), L.ptr(s.coef), ne, b, st),
                        "fv_jpeg_huff")
            L.check(lib.fv_jpeg_idct(L.ptr(s.coef), ne, L.ptr(s.table), L.ptr(self._planes), ne, b, st), "fv_jpeg_idct")
        L.check(lib.fv_jpeg_rgb(L.ptr(self._planes), ne, L.ptr(s.table), L.ptr(s.pool), ctypes.c_longlong(self.capacity), b, st),
                "fv_jpeg_rgb")
        self._record(s)

    def stream_status(self):
        """The status word of every sample of the slot committed last, as ``fv_jpeg_huff`` left them: (batch,) int32 on the
        host, 0 for a sample whose lanes all finished (1: bad Huffman code, 2: run past 63, 3: coefficient capacity, 4: a
        record or entry that does not fit).  A device-to-host copy: for diagnosis, not for the step path."""
        s = self._ready
        if s is None or not self.stream_bytes:
            raise RuntimeError("JpegImageStage.stream_status: no indexed batch was committed")
        huff = s.stable[:self.batch * SREC_INTS].view(self.batch, SREC_INTS)[:, 24].cpu()
        if not self.sync:
            return huff
        # a sample fv_jpeg_sync gave up on (5: a job that does not fit, 6: the states turn invalid before the last group
        # start needed) reports that, not the FV_JPEG_ST_RECORD its unwritten entries then give fv_jpeg_huff's lanes
        sync = s.sync.view(self.batch, SYNC_JOB_INTS)[:, 24].cpu()
        return torch.where(sync != 0, sync, huff)

    def sync_rounds(self):
        """The rounds of the fixed point that changed a state, per sample of the slot committed last, as ``fv_jpeg_sync``
        left them: (batch,) int32 on the host, 0 for a sample without a sync job.  A diagnostic: it synchronises, and
        ``resample`` never calls it."""
        s = self._ready
        if s is None or not self.sync:
            raise RuntimeError("JpegImageStage.sync_rounds: no batch of a sync=True stage was committed")
        return s.sync.view(self.batch, SYNC_JOB_INTS)[:, 25].cpu()

    def region(self, i):
        """The (h, w, 3) uint8 device view of sample ``i``'s source rectangle in the pool of the slot committed last."""
        s = self._ready
        h, w = (int(v) for v in s.host.plan[i, 2:4])
        off = s.host.offset(i)
        return s.pool[off:off + h * w * 3].view(h, w, 3)

    def resample(self, out):
        """``decode()``, then the two resample launches, into ``out`` (batch, 3, S_h, S_w) uint8."""
        self.decode()
        return super().resample(out)
