"""Device-side geometry of the uint8 loaders: the bicubic crop-and-resize and the horizontal flip of the MAE and linear-probe
training loaders (``RandomResizedCropAndInterpolation`` + ``RandomHorizontalFlip``: mae/datasets_mae.py:83-99) and the
``Resize`` + ``CenterCrop`` of every validation loader (imagenet_classification/datasets_supervised.py:254-262,
mae/datasets_finetune.py:254-270), computed on the GPU bit for bit as PIL computes them (csrc/resample.hip restates PIL's
8-bit ``ImagingResample``; include/fastvim_hip.h at ``fv_resample_coeffs``).

The host decodes, DRAWS the geometry and stages only the source rectangle of each sample; the device resamples straight
into the step's static uint8 input buffer, which ``fastvim_amd.pixels`` normalises inside the patch unfold::

    stage = ImageStage(B, 224, capacity_bytes=B * 1 << 20)
    for k, img in enumerate(decoded):                      # np.uint8 HWC, any sizes
        i, j, h, w, f = rrc.draw(*img.shape[:2]); stage.put(k, img, crop=(i, j, h, w), flip=f)
    stage.commit(); stage.resample(out=x_u8)               # x_u8: the step's static uint8 buffer
    step.step()                                            # or model(x_u8, mask_ratio=0.75) for MAE

``RandomResizedCrop`` is timm's draw (Python's ``random``, torchvision's flip on torch's CPU generator) without the pixels;
``ResizeCenterCrop`` is the validation plan.  The supervised / fine-tune TRAINING loaders run RandAugment on the crop: they
resample into a temporary buffer and ``fastvim_amd.randaug.RandAugment.apply`` augments it on the device into ``x_u8``.

The plan (one row of ``PLAN_INTS`` int32 per sample) and the pool live in device memory and are read when the launches
RUN: captured in a graph (``slots=1``: one device pool, one address) they resample what the last ``commit()`` put there.
A sample outside the kernels' range (more than 16x reduction on an axis, a side above 16384) is resized on the host with
PIL -- identical by construction -- and staged as an identity resample; ``last_fallbacks`` counts them."""
import ctypes
import math
import random

import numpy as np
import torch

from . import _lib as L

PLAN_INTS = 12            # FV_RESAMPLE_PLAN_INTS
MAX_TAPS = 65             # FV_RESAMPLE_MAX_TAPS
ALIGN = 16                # every staged sample starts on a 16-byte boundary of the pool


def _pair(v):
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"expected a size or (height, width), got {v!r}")
        return int(v[0]), int(v[1])
    return int(v), int(v)


def served(batch, s_h, s_w, h_src, w_src, o_h, o_w, win_y, win_x):
    """The range the kernels serve, restated in Python (``fv_resample_u8_ok`` of the library is the one the launcher
    uses; tests hold the two together): ``batch <= 4096``, window sides in [8, 1024], source sides in [1, 16384], output
    sides up to 65536, the window inside the output, at most 65 filter taps per axis (``src <= 16 out``)."""
    if not (1 <= batch <= 4096 and 8 <= s_h <= 1024 and 8 <= s_w <= 1024):
        return False
    if not (1 <= h_src <= 16384 and 1 <= w_src <= 16384 and 1 <= o_h <= 65536 and 1 <= o_w <= 65536):
        return False
    if win_y < 0 or win_x < 0 or win_y + s_h > o_h or win_x + s_w > o_w:
        return False
    return h_src <= 16 * o_h and w_src <= 16 * o_w


def resample_ok(batch, s_h, s_w, h_src, w_src, o_h, o_w, win_y, win_x):
    """``fv_resample_u8_ok``: host code of the library, the predicate its launcher applies."""
    return bool(L.lib().fv_resample_u8_ok(*(L.i32(v) for v in (batch, s_h, s_w, h_src, w_src, o_h, o_w, win_y, win_x))))


def workspace_ints(batch, s_h, s_w):
    return (s_h + s_w) * (2 + MAX_TAPS) * batch


# ---------------------------------------------------------------------------------------------------------------- draws
class RandomResizedCrop:
    """The DRAW of timm's ``RandomResizedCropAndInterpolation(size, scale, ratio)`` followed by torchvision's
    ``RandomHorizontalFlip(hflip)``: ``draw(H, W) -> (i, j, h, w, flip)``.  The box consumes Python's ``random`` in timm's
    order; the flip is ``torch.rand(1) < hflip`` on the CPU default generator (or ``generator=``) and is not drawn at all
    when ``hflip == 0`` (the loader then has no flip transform)."""

    def __init__(self, size, scale=(0.08, 1.0), ratio=(3. / 4., 4. / 3.), hflip=0.5, generator=None):
        self.size = _pair(size)
        self.scale, self.ratio = (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1]))
        self.hflip, self.generator = float(hflip), generator

    def box(self, H, W):
        area = H * W
        for _ in range(10):
            target_area = random.uniform(*self.scale) * area
            log_ratio = (math.log(self.ratio[0]), math.log(self.ratio[1]))
            aspect_ratio = math.exp(random.uniform(*log_ratio))
            w = int(round(math.sqrt(target_area * aspect_ratio)))
            h = int(round(math.sqrt(target_area / aspect_ratio)))
            if w <= W and h <= H:
                i = random.randint(0, H - h)
                j = random.randint(0, W - w)
                return i, j, h, w
        in_ratio = W / H
        if in_ratio < min(self.ratio):
            w = W
            h = int(round(w / min(self.ratio)))
        elif in_ratio > max(self.ratio):
            h = H
            w = int(round(h * max(self.ratio)))
        else:
            w, h = W, H
        return (H - h) // 2, (W - w) // 2, h, w

    def draw(self, H, W):
        i, j, h, w = self.box(int(H), int(W))
        flip = False
        if self.hflip > 0:
            flip = bool(torch.rand(1, generator=self.generator) < self.hflip)
        return i, j, h, w, flip


class ResizeCenterCrop:
    """The validation geometry: ``Resize(int(img_size / crop_ratio), bicubic)`` -- torchvision's: the short side to that
    size, the long side to ``int(size * long / short)`` -- then ``CenterCrop(img_size)``; ``crop_ratio`` is 1.0 above
    224 px, as in the reference's loaders.  ``plan(H, W) -> ((o_h, o_w), (win_y, win_x))`` for ``ImageStage.put``."""

    def __init__(self, img_size, crop_ratio=0.875):
        self.img_size = int(img_size)
        self.crop_ratio = 1.0 if self.img_size > 224 else float(crop_ratio)
        self.size = int(self.img_size / self.crop_ratio)

    def plan(self, H, W):
        H, W, size = int(H), int(W), self.size
        if W <= H:
            o_w, o_h = size, int(size * H / W)
        else:
            o_h, o_w = size, int(size * W / H)
        if o_h < self.img_size or o_w < self.img_size:
            raise ValueError(f"ResizeCenterCrop: the {o_h}x{o_w} resize of a {H}x{W} image is smaller than the {self.img_size} px crop")
        win_y = int(round((o_h - self.img_size) / 2.0))
        win_x = int(round((o_w - self.img_size) / 2.0))
        return (o_h, o_w), (win_y, win_x)


# ---------------------------------------------------------------------------------------------------------- host staging
def _pil_resize(a, o_h, o_w):
    from PIL import Image
    return np.asarray(Image.fromarray(a).resize((o_w, o_h), Image.BICUBIC))


class HostPlan:
    """The host half of one ring slot, plain numpy (no GPU): the byte pool the source rectangles are packed into, each
    starting 16-byte aligned, and the plan table.  ``pool`` (uint8) and ``plan`` (batch, PLAN_INTS) int32 may be views of
    pinned memory."""

    def __init__(self, batch, out_size, capacity_bytes, pool=None, plan=None):
        self.batch, (self.s_h, self.s_w) = int(batch), _pair(out_size)
        self.capacity = int(capacity_bytes)
        if not served(self.batch, self.s_h, self.s_w, self.s_h, self.s_w, self.s_h, self.s_w, 0, 0):
            raise ValueError(f"ImageStage: batch {self.batch} with a {self.s_h}x{self.s_w} window is outside the kernels' range "
                             "(batch <= 4096, sides in [8, 1024])")
        self.pool = np.zeros(self.capacity, np.uint8) if pool is None else pool
        self.plan = np.zeros((self.batch, PLAN_INTS), np.int32) if plan is None else plan
        assert self.pool.shape == (self.capacity,) and self.plan.shape == (self.batch, PLAN_INTS)
        self.reset()

    def reset(self):
        self.used = 0                          # bytes of the pool in use
        self.filled = [False] * self.batch
        self.fallbacks = 0

    def put(self, i, a, crop=None, out_full=None, window=(0, 0), flip=False):
        if not 0 <= i < self.batch:
            raise IndexError(f"ImageStage.put: sample {i} of a batch of {self.batch}")
        if self.filled[i]:
            raise ValueError(f"ImageStage.put: sample {i} was already put in this batch")
        a = np.asarray(a)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"ImageStage.put: sample {i} must be an (H, W, 3) uint8 array, got {a.dtype} {a.shape}")
        if crop is not None:
            ci, cj, ch, cw = (int(v) for v in crop)
            if min(ci, cj) < 0 or ch < 1 or cw < 1 or ci + ch > a.shape[0] or cj + cw > a.shape[1]:
                raise ValueError(f"ImageStage.put: crop {tuple(crop)} of sample {i} does not lie inside its {a.shape[0]}x{a.shape[1]} image")
            a = a[ci:ci + ch, cj:cj + cw]
        h, w = a.shape[:2]
        if h < 1 or w < 1:
            raise ValueError(f"ImageStage.put: sample {i} is empty")
        o_h, o_w = (self.s_h, self.s_w) if out_full is None else _pair(out_full)
        win_y, win_x = (int(v) for v in window)
        if o_h < 1 or o_w < 1 or win_y < 0 or win_x < 0 or win_y + self.s_h > o_h or win_x + self.s_w > o_w:
            raise ValueError(f"ImageStage.put: the {self.s_h}x{self.s_w} window at {(win_y, win_x)} of sample {i} does not lie "
                             f"inside its {o_h}x{o_w} resize")
        if not resample_ok(self.batch, self.s_h, self.s_w, h, w, o_h, o_w, win_y, win_x):
            # beyond the kernels' range: PIL itself on the host, staged as an identity resample -- flip and all that
            # follows stay on the device
            try:
                a = _pil_resize(np.ascontiguousarray(a), o_h, o_w)
            except ImportError:
                raise ValueError(f"ImageStage.put: sample {i} ({h}x{w} -> {o_h}x{o_w}, scale {max(h / o_h, w / o_w):.2f}) is outside "
                                 "the device range (at most 16x reduction, sides up to 16384) and PIL is not importable for "
                                 "the host fallback") from None
            a = a[win_y:win_y + self.s_h, win_x:win_x + self.s_w]
            h, w, o_h, o_w, win_y, win_x = self.s_h, self.s_w, self.s_h, self.s_w, 0, 0
            self.fallbacks += 1
        off = self.reserve(i, h, w, o_h, o_w, win_y, win_x, flip)
        np.copyto(self.pool[off:off + h * w * 3].reshape(h, w, 3), a)
        return off

    def reserve(self, i, h, w, o_h, o_w, win_y, win_x, flip):
        """Take the next ``h * w * 3`` bytes of the pool for sample ``i`` and write its plan row; the caller fills the
        region -- ``put`` from the decoded array, ``fastvim_amd.jpeg`` on the device."""
        off = (self.used + ALIGN - 1) // ALIGN * ALIGN
        nbytes = h * w * 3
        if off + nbytes > self.capacity:
            raise ValueError(f"ImageStage.put: sample {i} ({nbytes} bytes at offset {off}) overflows capacity_bytes = {self.capacity}")
        self.plan[i] = (0, 0, h, w, o_h, o_w, win_y, win_x, int(bool(flip)), 0, 0, 0)
        self.plan.view(np.uint32)[i, :2] = (off & 0xffffffff, off >> 32)      # the byte offset as 64 bits, low word first
        self.used = off + nbytes
        self.filled[i] = True
        return off

    def offset(self, i):
        lo, hi = (int(v) for v in self.plan.view(np.uint32)[i, :2])
        return lo | (hi << 32)

    def check_complete(self):
        missing = [i for i, f in enumerate(self.filled) if not f]
        if missing:
            raise RuntimeError(f"ImageStage.commit: samples {missing[:8]}{'...' if len(missing) > 8 else ''} of the batch were never put")


class _Slot:
    def __init__(self, batch, out_size, capacity, device):
        self.pool_pin = torch.zeros(capacity, dtype=torch.uint8).pin_memory()
        self.plan_pin = torch.zeros(batch, PLAN_INTS, dtype=torch.int32).pin_memory()
        self.host = HostPlan(batch, out_size, capacity, pool=self.pool_pin.numpy(), plan=self.plan_pin.numpy())
        self.pool = torch.zeros(capacity, dtype=torch.uint8, device=device)
        self.plan = torch.zeros(batch, PLAN_INTS, dtype=torch.int32, device=device)
        self.event = None                      # after the last copy out of / launch on this slot


class ImageStage:
    """Pinned host pools and device pools as a ring of ``slots``, the plan tables and the coefficient workspace of a batch
    of ``batch`` images resampled to ``out_size`` (a side or ``(S_h, S_w)``).

    ``put`` fills the current slot on the host; ``commit()`` enqueues its two asynchronous copies (pool, plan) on the
    current stream and moves on to the next slot; ``resample(out=x)`` runs the two launches on the slot committed last.
    A slot is filled again only after its own copies and the launches that read it are done (an event per slot, waited
    for by the first ``put`` that returns to it), so ``slots=2`` lets the host stage batch n + 1 while batch n is in flight.
    With ``slots=1`` the device addresses never change: ``resample`` can be captured in a graph and replayed after every
    ``commit()``."""

    def __init__(self, batch, out_size, capacity_bytes, slots=2, device=None):
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("fastvim_amd ops run on the GPU only (HIP kernels); ImageStage needs a GPU device")
        if slots < 1:
            raise ValueError("ImageStage: at least one slot")
        self.batch, (self.s_h, self.s_w) = int(batch), _pair(out_size)
        self.capacity = (int(capacity_bytes) + ALIGN - 1) // ALIGN * ALIGN
        self.device = device
        self._slots = [_Slot(self.batch, (self.s_h, self.s_w), self.capacity, device) for _ in range(int(slots))]
        n = int(L.lib().fv_resample_workspace_ints(L.i32(self.batch), L.i32(self.s_h), L.i32(self.s_w)))
        assert n == workspace_ints(self.batch, self.s_h, self.s_w)
        self._ws = torch.empty(n, dtype=torch.int32, device=device)
        self._fill = 0                         # the slot being filled
        self._open = False                     # a put since the last commit
        self._ready = None                     # the slot committed last
        self.last_fallbacks = 0
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

    def put(self, i, array_hwc_u8, crop=None, out_full=None, window=(0, 0), flip=False):
        """Stage sample ``i``: the ``crop = (top, left, h, w)`` rectangle of the decoded image (default: all of it), to be
        resized to ``out_full = (o_h, o_w)`` (default: the stage's output size), of which the output-sized window at
        ``window = (win_y, win_x)`` is written, mirrored if ``flip``."""
        s = self._filling()
        s.host.put(int(i), array_hwc_u8, crop=crop, out_full=out_full, window=window, flip=flip)

    def commit(self):
        s = self._filling()
        s.host.check_complete()
        self._copy_pool(s)
        s.plan.copy_(s.plan_pin, non_blocking=True)
        self._record(s)
        self.last_fallbacks = s.host.fallbacks
        self.staged_bytes = s.host.used
        self._ready = s
        self._open = False
        self._fill = (self._fill + 1) % len(self._slots)

    def _copy_pool(self, s):
        """The pool bytes the host filled, to the device (``JpegImageStage`` leaves out what the device fills itself)."""
        used = (s.host.used + ALIGN - 1) // ALIGN * ALIGN
        s.pool[:used].copy_(s.pool_pin[:used], non_blocking=True)

    def _record(self, s):
        if torch.cuda.is_current_stream_capturing():
            return                             # a replayed launch is ordered by the stream the graph is replayed on
        s.event = torch.cuda.Event()
        s.event.record(torch.cuda.current_stream(self.device))

    def resample(self, out):
        """The two launches (coefficients, then pixels) on the slot committed last, into ``out`` (batch, 3, S_h, S_w) uint8."""
        s = self._ready
        if s is None:
            raise RuntimeError("ImageStage.resample: nothing was committed")
        L.require_gpu(out)
        if out.dtype != torch.uint8 or tuple(out.shape) != (self.batch, 3, self.s_h, self.s_w) or not out.is_contiguous():
            raise ValueError(f"ImageStage.resample: out must be a contiguous uint8 ({self.batch}, 3, {self.s_h}, {self.s_w}) "
                             f"tensor, got {out.dtype} {tuple(out.shape)}")
        if out.device != self.device:
            raise RuntimeError(f"ImageStage: the pools live on {self.device}, out on {out.device}")
        lib, st = L.lib(), L.stream_of(out)
        nbytes = ctypes.c_longlong(self.capacity)
        b, sh, sw = L.i32(self.batch), L.i32(self.s_h), L.i32(self.s_w)
        L.check(lib.fv_resample_coeffs(L.ptr(s.plan), nbytes, L.ptr(self._ws), b, sh, sw, st), "fv_resample_coeffs")
        L.check(lib.fv_resample_u8(L.ptr(s.pool), nbytes, L.ptr(s.plan), L.ptr(self._ws), L.ptr(out), b, sh, sw, st), "fv_resample_u8")
        self._record(s)
        return out
