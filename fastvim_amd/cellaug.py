"""Device-side cell-image augmentation of the channel models' loader: the training transform of the reference's
``CellAugmentation(is_train=True)`` (cell_imaging/transformations/cell.py:104-149) in front of ``A.Normalize``, which
``fastvim_amd.pixels.attach_pixel_norm(..., formula="albumentations")`` computes inside ``fv_patch_unfold_chan_u8``.

The host DRAWS and copies, the device does the pixels (csrc/cellaug.hip; include/fastvim_hip.h at ``fv_cellaug_geom``)::

    aug = CellAugmentation(224, seed=rank)                   # recipe defaults; every probability / range is a keyword
    stage = CellStage(B, channels=8, out_size=224, capacity_bytes=B << 19, slots=2)
    for k, img in enumerate(cells):                          # np.uint8 (C, H, W) as the .npy holds it, any H, W
        stage.put(k, img, aug.draw(img.shape[1], img.shape[2]))
    stage.commit(); stage.apply(out=x_u8)                    # x_u8: (B, 8, 224, 224) uint8, the step's static buffer
    sampler.sample(); step.step()
    stage.put(k, img, None)                                  # validation: identity, H = W = out_size or ValueError

The recipe, in order: ``PadIfNeeded(256, 256, position="random", constant 0)`` + ``RandomCrop(S, S)``; with probability
0.5 one of {HorizontalFlip, VerticalFlip, Rotate(limit=90), Rotate(limit=180), Rotate(limit=270)} -- the three rotations
are by a uniformly drawn ANGLE about the crop's centre, bilinear, reflect-101 within the crop; ``Defocus(radius=(1, 3),
alias_blur=(0.1, 0.5))`` with probability 0.5; ``CoarseDropout(10, 10, 10)`` with probability 0.5.

The DISTRIBUTIONS are the recipe's; the random STREAM is this project's own (albumentations is not a dependency, and its
stream differs between its versions).  Nothing more is claimed: the rotation restates the published fixed-point scheme of an
8-bit bilinear ``warpAffine`` and the defocus a float correlation in a fixed order -- tests hold both to scipy within
derived bounds, not to OpenCV's bytes.

The plan table (one record of ``PLAN_INTS`` int32 per sample) and the pool live in device memory and are read when the
launches RUN: captured in a graph (``slots=1``) they augment what the last ``commit()`` put there."""
import ctypes
import math
import random

import numpy as np
import torch

from . import _lib as L

PLAN_INTS = 176           # FV_CELLAUG_PLAN_INTS
TAPS = 9                  # FV_CELLAUG_TAPS: the defocus support the device serves (radius <= 3)
MAX_RADIUS = (TAPS - 1) // 2 - 1
MAX_HOLES = 16            # FV_CELLAUG_MAX_HOLES
ALIGN = 16                # every staged sample starts on a 16-byte boundary of the pool
NONE, HFLIP, VFLIP, ROTATE = 0, 1, 2, 3
# words of a record (include/fastvim_hip.h, THE CELL RECORD)
_R_MATRIX, _R_KERNEL, _R_HOLES = 12, 24, 108


# ------------------------------------------------------------------------------------------- draws turned into numbers
def rotation_matrix(size, angle):
    """The six fp64 entries of the inverse (destination to source) map of a rotation by ``angle`` degrees about the
    centre of a ``size`` x ``size`` crop: ``getRotationMatrix2D((S/2 - 0.5, S/2 - 0.5), angle, 1)`` followed by the closed
    form of the affine inverse that ``warpAffine`` applies to a forward matrix."""
    c = size / 2 - 0.5
    a = float(angle) * (math.pi / 180.0)
    alpha, beta = math.cos(a), math.sin(a)
    m0, m1, m2 = alpha, beta, (1 - alpha) * c - beta * c
    m3, m4, m5 = -beta, alpha, beta * c + (1 - alpha) * c
    d = m0 * m4 - m1 * m3
    d = 1.0 / d if d != 0 else 0.0
    a11, a22 = m4 * d, m0 * d
    m0, m1, m3, m4 = a11, m1 * -d, m3 * -d, a22
    b1 = -m0 * m2 - m1 * m5
    b2 = -m3 * m2 - m4 * m5
    return (m0, m1, b1, m3, m4, b2)


def defocus_kernel_full(radius, sigma):
    """The recipe's 17 x 17 defocus kernel in numpy fp32: the disk ``(X^2 + Y^2 <= r^2) / count`` blurred by the separable
    3-tap Gaussian ``exp(-x^2 / (2 sigma^2))`` (normalised in fp64, applied in fp32: rows, then columns; the disk does
    not reach the border for r <= 6, so the border rule does not matter)."""
    radius = int(radius)
    if radius < 1:
        raise ValueError(f"defocus radius {radius}: at least 1")
    n = max(8, radius)
    ax = np.arange(-n, n + 1)
    xx, yy = np.meshgrid(ax, ax)
    disk = (xx ** 2 + yy ** 2 <= radius ** 2).astype(np.float32)
    disk /= np.sum(disk, dtype=np.float32)
    g = np.exp(-np.array([1.0, 0.0, 1.0]) / (2.0 * float(sigma) ** 2))
    g = (g / g.sum()).astype(np.float32)
    p = np.pad(disk, ((0, 0), (1, 1)))
    rows = (p[:, :-2] * g[0] + p[:, 1:-1] * g[1]).astype(np.float32) + p[:, 2:] * g[2]
    p = np.pad(rows.astype(np.float32), ((1, 1), (0, 0)))
    out = (p[:-2] * g[0] + p[1:-1] * g[1]).astype(np.float32) + p[2:] * g[2]
    return np.ascontiguousarray(out, dtype=np.float32)


def defocus_kernel(radius, sigma):
    """The central 9 x 9 of ``defocus_kernel_full`` -- all of its non-zero support for a radius up to 3, which is what the
    device serves; a larger radius raises."""
    if int(radius) > MAX_RADIUS:
        raise ValueError(f"defocus radius {radius}: the device serves a {TAPS} x {TAPS} support (radius <= {MAX_RADIUS})")
    k = defocus_kernel_full(radius, sigma)
    c, h = k.shape[0] // 2, TAPS // 2
    assert np.count_nonzero(k) == np.count_nonzero(k[c - h:c + h + 1, c - h:c + h + 1])
    return np.ascontiguousarray(k[c - h:c + h + 1, c - h:c + h + 1])


class CellPlan:
    """What one sample's draw decided; no pixels.  ``oy, ox``: crop pixel (y, x) is ``src[:, y - oy, x - ox]`` inside the
    source and 0 outside (pad offset minus crop origin).  ``op``: NONE, HFLIP, VFLIP or ROTATE (by ``angle`` degrees).
    ``radius`` / ``sigma``: the defocus, or ``radius = 0`` for none.  ``holes``: ``(y1, x1, y2, x2)`` rectangles, ends
    exclusive.  Tests build plans directly; ``CellAugmentation.draw`` draws them."""
    __slots__ = ("oy", "ox", "op", "angle", "radius", "sigma", "holes")

    def __init__(self, oy=0, ox=0, op=NONE, angle=0.0, radius=0, sigma=0.0, holes=()):
        self.oy, self.ox, self.op, self.angle = int(oy), int(ox), int(op), float(angle)
        self.radius, self.sigma = int(radius), float(sigma)
        self.holes = tuple(tuple(int(v) for v in h) for h in holes)

    def __eq__(self, other):
        return isinstance(other, CellPlan) and all(getattr(self, s) == getattr(other, s) for s in self.__slots__)

    def __repr__(self):
        return "CellPlan(" + ", ".join(f"{s}={getattr(self, s)!r}" for s in self.__slots__) + ")"


class CellAugmentation:
    """The DRAW of the recipe for an ``out_size`` crop: ``draw(H, W) -> CellPlan``; no pixel work.

    Draws come from a ``random.Random(seed)`` of its own in this fixed order (a step that does not fire draws nothing
    more): pad top ``randint(0, max(min_side, H) - H)``, pad left likewise; crop top ``randint(0, canvas_h - S)``, crop
    left; ``random() < p_flip_rotate``, then the member ``randrange(5)`` (0 horizontal flip, 1 vertical flip, 2 / 3 / 4
    rotation with ``rotate_limits[member - 2]``) and for a rotation ``uniform(-limit, limit)``; ``random() < p_defocus``,
    then ``randint(*radius)`` and ``uniform(*alias_blur)``; ``random() < p_dropout``, then the number of holes
    ``randint(min_holes, max_holes)`` and per hole its height ``randint(min_height, max_height)``, width, top
    ``randint(0, S - height)`` and left.  ``min_*`` left at ``None`` equal the maximum, as in albumentations 1.3.

    The distributions are the recipe's; the stream is this project's own, not albumentations'."""

    def __init__(self, out_size=224, seed=None, min_side=256, p_flip_rotate=0.5, rotate_limits=(90, 180, 270), p_defocus=0.5,
                 radius=(1, 3), alias_blur=(0.1, 0.5), p_dropout=0.5, max_holes=10, max_height=10, max_width=10,
                 min_holes=None, min_height=None, min_width=None):
        self.size, self.min_side = int(out_size), int(min_side)
        self.p_flip_rotate, self.p_defocus, self.p_dropout = float(p_flip_rotate), float(p_defocus), float(p_dropout)
        self.rotate_limits = tuple(float(v) for v in rotate_limits)
        self.radius = (int(radius[0]), int(radius[1]))
        self.alias_blur = (float(alias_blur[0]), float(alias_blur[1]))
        self.holes = (int(max_holes if min_holes is None else min_holes), int(max_holes))
        self.hole_h = (int(max_height if min_height is None else min_height), int(max_height))
        self.hole_w = (int(max_width if min_width is None else min_width), int(max_width))
        if len(self.rotate_limits) != 3:
            raise ValueError("CellAugmentation: three rotation limits (the recipe's Rotate(90), Rotate(180), Rotate(270))")
        if not 1 <= self.radius[0] <= self.radius[1]:
            raise ValueError(f"CellAugmentation: defocus radius range {self.radius}")
        if self.radius[1] > MAX_RADIUS:
            raise ValueError(f"CellAugmentation: defocus radius {self.radius[1]}: the device serves a {TAPS} x {TAPS} support "
                             f"(radius <= {MAX_RADIUS})")
        if not 0 < self.alias_blur[0] <= self.alias_blur[1]:
            raise ValueError(f"CellAugmentation: alias_blur range {self.alias_blur}")
        if not 0 <= self.holes[0] <= self.holes[1] <= MAX_HOLES:
            raise ValueError(f"CellAugmentation: {self.holes} holes: the device serves up to {MAX_HOLES}")
        for lo, hi in (self.hole_h, self.hole_w):
            if not 1 <= lo <= hi <= self.size:
                raise ValueError(f"CellAugmentation: hole sides {lo}..{hi} for a {self.size} px crop")
        self.rng = random.Random(seed)

    def draw(self, H, W):
        H, W, S, r = int(H), int(W), self.size, self.rng
        canvas_h, canvas_w = max(self.min_side, H), max(self.min_side, W)
        if canvas_h < S or canvas_w < S:
            raise ValueError(f"CellAugmentation.draw: a {S} px crop of the {canvas_h}x{canvas_w} canvas of a {H}x{W} image")
        pad_top, pad_left = r.randint(0, canvas_h - H), r.randint(0, canvas_w - W)
        crop_top, crop_left = r.randint(0, canvas_h - S), r.randint(0, canvas_w - S)
        op, angle = NONE, 0.0
        if r.random() < self.p_flip_rotate:
            member = r.randrange(5)
            if member < 2:
                op = HFLIP if member == 0 else VFLIP
            else:
                limit = self.rotate_limits[member - 2]
                op, angle = ROTATE, r.uniform(-limit, limit)
        radius, sigma = 0, 0.0
        if r.random() < self.p_defocus:
            radius, sigma = r.randint(*self.radius), r.uniform(*self.alias_blur)
        holes = []
        if r.random() < self.p_dropout:
            for _ in range(r.randint(*self.holes)):
                h, w = r.randint(*self.hole_h), r.randint(*self.hole_w)
                y1, x1 = r.randint(0, S - h), r.randint(0, S - w)
                holes.append((y1, x1, y1 + h, x1 + w))
        return CellPlan(pad_top - crop_top, pad_left - crop_left, op, angle, radius, sigma, holes)


# ---------------------------------------------------------------------------------------------------------- host staging
def write_record(row, plan, size, off, h, w):
    """One record of the plan table (THE CELL RECORD of include/fastvim_hip.h) into ``row``, ``PLAN_INTS`` int32."""
    if plan.op not in (NONE, HFLIP, VFLIP, ROTATE):
        raise ValueError(f"CellStage.put: geometry op {plan.op}")
    if abs(plan.oy) > 8192 or abs(plan.ox) > 8192:
        raise ValueError(f"CellStage.put: crop offset {(plan.oy, plan.ox)} outside +-8192")
    if len(plan.holes) > MAX_HOLES:
        raise ValueError(f"CellStage.put: {len(plan.holes)} holes, the device serves up to {MAX_HOLES}")
    row[:] = 0
    row.view(np.uint32)[:2] = (off & 0xffffffff, off >> 32)
    row[2:9] = (h, w, plan.oy, plan.ox, plan.op, int(plan.radius > 0), len(plan.holes))
    if plan.op == ROTATE:
        if not math.isfinite(plan.angle):
            raise ValueError(f"CellStage.put: rotation angle {plan.angle}")
        row[_R_MATRIX:_R_MATRIX + 12].view(np.float64)[:] = rotation_matrix(size, plan.angle)
    if plan.radius > 0:
        if not (plan.sigma > 0 and math.isfinite(plan.sigma)):
            raise ValueError(f"CellStage.put: defocus alias blur (sigma) {plan.sigma}: a positive number")
        row[_R_KERNEL:_R_KERNEL + TAPS * TAPS].view(np.float32)[:] = defocus_kernel(plan.radius, plan.sigma).reshape(-1)
    for k, (y1, x1, y2, x2) in enumerate(plan.holes):
        if not (0 <= y1 <= y2 <= size and 0 <= x1 <= x2 <= size):
            raise ValueError(f"CellStage.put: hole {(y1, x1, y2, x2)} does not lie inside the {size} px crop")
        row[_R_HOLES + 4 * k:_R_HOLES + 4 * k + 4] = (y1, x1, y2, x2)


def read_record(row):
    """The inverse of ``write_record`` as plain values: ``(off, h, w, oy, ox, op, matrix, kernel or None, holes)``."""
    row = np.ascontiguousarray(row, dtype=np.int32)
    lo, hi = (int(v) for v in row.view(np.uint32)[:2])
    h, w, oy, ox, op, defocus, nh = (int(v) for v in row[2:9])
    matrix = tuple(float(v) for v in row[_R_MATRIX:_R_MATRIX + 12].view(np.float64))
    kernel = row[_R_KERNEL:_R_KERNEL + TAPS * TAPS].view(np.float32).reshape(TAPS, TAPS).copy() if defocus else None
    holes = tuple(tuple(int(v) for v in row[_R_HOLES + 4 * k:_R_HOLES + 4 * k + 4]) for k in range(nh))
    return lo | (hi << 32), h, w, oy, ox, op, matrix, kernel, holes


class HostCellPlan:
    """The host half of one ring slot, plain numpy (no GPU): the byte pool the (C, H, W) sources are packed into, each
    starting 16-byte aligned, and the plan table.  ``pool`` (uint8) and ``plan`` (batch, PLAN_INTS) int32 may be views of
    pinned memory."""

    def __init__(self, batch, channels, out_size, capacity_bytes, pool=None, plan=None):
        self.batch, self.channels, self.size = int(batch), int(channels), int(out_size)
        self.capacity = int(capacity_bytes)
        if not (1 <= self.batch <= 4096 and 1 <= self.channels <= 16 and 8 <= self.size <= 512):
            raise ValueError(f"CellStage: batch {self.batch}, channels {self.channels}, out_size {self.size} outside the kernels' "
                             "range (batch <= 4096, channels in [1, 16], out_size in [8, 512])")
        self.pool = np.zeros(self.capacity, np.uint8) if pool is None else pool
        self.plan = np.zeros((self.batch, PLAN_INTS), np.int32) if plan is None else plan
        assert self.pool.shape == (self.capacity,) and self.plan.shape == (self.batch, PLAN_INTS)
        self.reset()

    def reset(self):
        self.used = 0
        self.filled = [False] * self.batch

    def put(self, i, a, plan=None):
        if not 0 <= i < self.batch:
            raise IndexError(f"CellStage.put: sample {i} of a batch of {self.batch}")
        if self.filled[i]:
            raise ValueError(f"CellStage.put: sample {i} was already put in this batch")
        a = np.asarray(a)
        if a.dtype != np.uint8 or a.ndim != 3:
            raise ValueError(f"CellStage.put: sample {i} must be a (C, H, W) uint8 array, got {a.dtype} {a.shape}")
        c, h, w = a.shape
        if c != self.channels:
            raise ValueError(f"CellStage.put: sample {i} has {c} channels, the stage {self.channels}")
        if not (1 <= h <= 4096 and 1 <= w <= 4096):
            raise ValueError(f"CellStage.put: sample {i} is {h}x{w}, source sides must lie in [1, 4096]")
        if plan is None:
            if (h, w) != (self.size, self.size):
                raise ValueError(f"CellStage.put: sample {i} is {h}x{w}; without a plan it must be {self.size}x{self.size}")
            plan = CellPlan()
        off = (self.used + ALIGN - 1) // ALIGN * ALIGN
        nbytes = c * h * w
        if off + nbytes > self.capacity:
            raise ValueError(f"CellStage.put: sample {i} ({nbytes} bytes at offset {off}) overflows capacity_bytes = {self.capacity}")
        write_record(self.plan[i], plan, self.size, off, h, w)
        np.copyto(self.pool[off:off + nbytes].reshape(c, h, w), a)
        self.used = off + nbytes
        self.filled[i] = True
        return off

    def check_complete(self):
        missing = [i for i, f in enumerate(self.filled) if not f]
        if missing:
            raise RuntimeError(f"CellStage.commit: samples {missing[:8]}{'...' if len(missing) > 8 else ''} of the batch were never put")


class _Slot:
    def __init__(self, batch, channels, out_size, capacity, device):
        self.pool_pin = torch.zeros(capacity, dtype=torch.uint8).pin_memory()
        self.plan_pin = torch.zeros(batch, PLAN_INTS, dtype=torch.int32).pin_memory()
        self.host = HostCellPlan(batch, channels, out_size, capacity, pool=self.pool_pin.numpy(), plan=self.plan_pin.numpy())
        self.pool = torch.zeros(capacity, dtype=torch.uint8, device=device)
        self.plan = torch.zeros(batch, PLAN_INTS, dtype=torch.int32, device=device)
        self.event = None                      # after the last copy out of / launch on this slot


def geom(pool, plan, out):
    """``fv_cellaug_geom``: the staged sources -> the (B, C, S, S) uint8 crop with its flip or rotation applied."""
    _check_planes("cellaug.geom", out, plan)
    L.require_gpu(pool, plan, out)
    if pool.dtype != torch.uint8 or pool.dim() != 1 or not pool.is_contiguous():
        raise ValueError("cellaug.geom: pool must be a contiguous 1-d uint8 tensor")
    b, c, s, _ = out.shape
    L.check(L.lib().fv_cellaug_geom(L.ptr(pool), ctypes.c_longlong(pool.numel()), L.ptr(plan), L.ptr(out), L.i32(b), L.i32(c),
                                    L.i32(s), L.stream_of(out)), "fv_cellaug_geom")
    return out


def filter(inp, plan, out):
    """``fv_cellaug_filter``: defocus (or copy) and holes, (B, C, S, S) uint8 -> ``out`` of the same shape."""
    _check_planes("cellaug.filter", out, plan)
    _check_planes("cellaug.filter", inp, plan)
    L.require_gpu(inp, plan, out)
    if inp.shape != out.shape:
        raise ValueError(f"cellaug.filter: in {tuple(inp.shape)} and out {tuple(out.shape)} differ")
    b, c, s, _ = out.shape
    L.check(L.lib().fv_cellaug_filter(L.ptr(inp), L.ptr(plan), L.ptr(out), L.i32(b), L.i32(c), L.i32(s), L.stream_of(out)),
            "fv_cellaug_filter")
    return out


def _check_planes(what, t, plan):
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[2] != t.shape[3] or not t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous uint8 (B, C, S, S) tensor, got {t.dtype} {tuple(t.shape)}")
    if plan.dtype != torch.int32 or tuple(plan.shape) != (t.shape[0], PLAN_INTS) or not plan.is_contiguous():
        raise ValueError(f"{what}: plan must be a contiguous int32 ({t.shape[0]}, {PLAN_INTS}) tensor, got {plan.dtype} {tuple(plan.shape)}")
    if plan.device != t.device:
        raise RuntimeError(f"{what}: the plan lives on {plan.device}, the planes on {t.device}")


class CellStage:
    """Pinned host pools and device pools as a ring of ``slots``, the plan tables and the scratch planes of a batch of
    ``batch`` cell images of ``channels`` planes augmented to ``out_size`` x ``out_size``.

    ``put`` fills the current slot on the host; ``commit()`` enqueues its two asynchronous copies (pool, plan) on the
    current stream and moves on to the next slot; ``apply(out=x)`` runs the two launches on the slot committed last.
    A slot is filled again only after its own copies and the launches that read it are done (an event per slot, waited
    for by the first ``put`` that returns to it), so ``slots=2`` lets the host stage batch n + 1 while batch n is in flight.
    With ``slots=1`` the device addresses never change: ``apply`` can be captured in a graph and replayed after every
    ``commit()``."""

    def __init__(self, batch, channels, out_size, capacity_bytes, slots=2, device=None):
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("fastvim_amd ops run on the GPU only (HIP kernels); CellStage needs a GPU device")
        if slots < 1:
            raise ValueError("CellStage: at least one slot")
        self.batch, self.channels, self.size = int(batch), int(channels), int(out_size)
        self.capacity = (int(capacity_bytes) + ALIGN - 1) // ALIGN * ALIGN
        self.device = device
        self._slots = [_Slot(self.batch, self.channels, self.size, self.capacity, device) for _ in range(int(slots))]
        self._scratch = torch.empty(self.batch, self.channels, self.size, self.size, dtype=torch.uint8, device=device)
        self._fill = 0                         # the slot being filled
        self._open = False                     # a put since the last commit
        self._ready = None                     # the slot committed last
        self.staged_bytes = 0                  # pool bytes of the batch committed last

    def _filling(self):
        s = self._slots[self._fill]
        if not self._open:
            if s.event is not None:
                s.event.synchronize()
                s.event = None
            s.host.reset()
            self._open = True
        return s

    def put(self, i, array_chw_u8, plan=None):
        """Stage sample ``i``: a (C, H, W) uint8 array and the ``CellPlan`` drawn for it; ``None`` is the identity and
        needs ``H = W = out_size`` (validation)."""
        self._filling().host.put(int(i), array_chw_u8, plan)

    def commit(self):
        s = self._filling()
        s.host.check_complete()
        used = (s.host.used + ALIGN - 1) // ALIGN * ALIGN
        s.pool[:used].copy_(s.pool_pin[:used], non_blocking=True)
        s.plan.copy_(s.plan_pin, non_blocking=True)
        self._record(s)
        self.staged_bytes = s.host.used
        self._ready = s
        self._open = False
        self._fill = (self._fill + 1) % len(self._slots)

    def _record(self, s):
        if torch.cuda.is_current_stream_capturing():
            return                             # a replayed launch is ordered by the stream the graph is replayed on
        s.event = torch.cuda.Event()
        s.event.record(torch.cuda.current_stream(self.device))

    def apply(self, out):
        """The two launches (geometry, then defocus + holes) on the slot committed last, into ``out`` (batch, channels, S, S)
        uint8."""
        s = self._ready
        if s is None:
            raise RuntimeError("CellStage.apply: nothing was committed")
        if tuple(out.shape) != tuple(self._scratch.shape):
            raise ValueError(f"CellStage.apply: out must be a uint8 {tuple(self._scratch.shape)} tensor, got {tuple(out.shape)}")
        if out.device != self.device:
            raise RuntimeError(f"CellStage: the pools live on {self.device}, out on {out.device}")
        geom(s.pool, s.plan, self._scratch)
        filter(self._scratch, s.plan, out)
        self._record(s)
        return out
