"""Device-side RandAugment of the supervised / fine-tune training loaders (``rand_augment_transform("rand-m9-mstd0.5-inc1",
aa_params)``: imagenet_classification/datasets_supervised.py:193-207, mae/datasets_finetune.py) on a planar uint8 batch,
byte for byte what timm's ``RandAugment`` computes with PIL on the same image with the same draws (csrc/randaug.hip
restates PIL's ``ImageOps`` / ``ImageEnhance`` / ``Image.transform``; include/fastvim_hip.h at ``fv_randaug_apply``).

The host DRAWS -- timm's consumption order of numpy's global legacy generator (one ``np.random.choice`` per image) and of
Python's ``random`` (per layer: the skip, the magnitude, the sign) -- and computes in Python what PIL's Python layer
computes (the affine coefficients as doubles); the device does the pixels, next to ``ImageStage.resample``::

    ra = RandAugment("rand-m9-mstd0.5-inc1", 224, IMAGENET_DEFAULT_MEAN, batch=B)
    for k, img in enumerate(decoded):
        i, j, h, w, f = rrc.draw(*img.shape[:2]); stage.put(k, img, crop=(i, j, h, w), flip=f); ra.draw(k)
    stage.commit(); ra.commit(); stage.resample(out=tmp); ra.apply(tmp, out=x_u8); step.step()

The plan (one record of ``PLAN_INTS`` int32 per sample and layer) lives at one device address and is read when the
launches RUN: ``apply`` captured in a graph augments by what the last ``commit()`` put there (the first ``commit()``
allocates the device buffers, so it comes before the capture).  Per layer there are two
launches: statistics (histograms of the samples whose op needs one) and apply.  There is no CPU form of ``apply``; the
numpy restatement the tests compare with is tests/randaug_ref.py."""
import math
import random
import re
import struct
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L

PLAN_INTS = 18            # FV_RANDAUG_PLAN_INTS
MAX_LAYERS = 4            # FV_RANDAUG_MAX_LAYERS
WS_BYTES = 768            # FV_RANDAUG_WS_BYTES per sample: a (3, 256) uint8 table
_LEVEL_DENOM = 10.

# FV_RA_*: what a record asks of the apply launch
(K_COPY, K_AUTOCONTRAST, K_EQUALIZE, K_INVERT, K_SOLARIZE, K_POSTERIZE, K_SOLARIZE_ADD, K_COLOR, K_CONTRAST, K_BRIGHTNESS,
 K_SHARPNESS, K_AFFINE) = range(12)

OPS = ("AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast",
       "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
OPS_INCREASING = ("AutoContrast", "Equalize", "Invert", "Rotate", "PosterizeIncreasing", "SolarizeIncreasing", "SolarizeAdd",
                  "ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing", "ShearX", "ShearY",
                  "TranslateXRel", "TranslateYRel")

Record = namedtuple("Record", "kind arg0 arg1 factor fill coeffs")
_IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def _pair(v):
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"expected a size or (height, width), got {v!r}")
        return int(v[0]), int(v[1])
    return int(v), int(v)


def served(batch, s_h, s_w, num_layers):
    """The range the launches serve, restated in Python (``fv_randaug_ok`` of the library is the one the launchers apply;
    tests hold the two together)."""
    return 1 <= batch <= 4096 and 8 <= s_h <= 1024 and 8 <= s_w <= 1024 and 1 <= num_layers <= MAX_LAYERS


def randaug_ok(batch, s_h, s_w, num_layers):
    """``fv_randaug_ok``: host code of the library."""
    return bool(L.lib().fv_randaug_ok(*(L.i32(v) for v in (batch, s_h, s_w, num_layers))))


# --------------------------------------------------------------------------------------------------------- the records
def pack_record(rec):
    """A record as ``PLAN_INTS`` int32: kind, arg0, arg1, the float32 bits of the factor, the fill colour (R | G << 8 |
    B << 16), 0, then the six doubles as twelve words, low word first."""
    r, g, b = (int(v) for v in rec.fill)
    words = struct.unpack("<6i", struct.pack("<3if2i", rec.kind, rec.arg0, rec.arg1, rec.factor, r | (g << 8) | (b << 16), 0))
    return np.array(words + struct.unpack("<12i", struct.pack("<6d", *rec.coeffs)), np.int32)


def unpack_record(words):
    raw = np.asarray(words, np.int32).tobytes()
    kind, arg0, arg1, factor, fill, _ = struct.unpack("<3if2i", raw[:24])
    return Record(kind, arg0, arg1, factor, (fill & 255, (fill >> 8) & 255, (fill >> 16) & 255), struct.unpack("<6d", raw[24:]))


def _randomly_negate(v):
    return -v if random.random() > 0.5 else v


def rotate_matrix(deg, W, H):
    """``Image.rotate(deg)``'s own matrix (centre of the image, no translation, no expand), or None where PIL returns a
    copy (``deg % 360 == 0``)."""
    deg = deg % 360.0
    if deg == 0:
        return None
    a = -math.radians(deg)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = W / 2.0, H / 2.0
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


class RandAugment:
    """timm's ``rand_augment_transform(config_str, dict(translate_const=..., img_mean=round(255 * mean), interpolation=
    BICUBIC))`` for a batch of ``batch`` images of ``img_size`` (a side or ``(S_h, S_w)``).  ``draw(k)`` fills the host
    plan of sample ``k``; ``commit()`` copies the plan to its fixed device address; ``apply(src, out)`` enqueues the
    launches.  Config keys ``m n p mstd mmax inc`` as in timm; ``w`` and ``t`` are not implemented."""

    def __init__(self, config_str, img_size, mean, batch, device=None):
        self.batch, (self.s_h, self.s_w) = int(batch), _pair(img_size)
        self.fill = tuple(min(255, round(255 * x)) for x in mean)
        if len(self.fill) != 3:
            raise ValueError(f"RandAugment: mean must have three channels, got {mean!r}")
        self.magnitude, self.num_layers, self.prob = 10, 2, 0.5
        self.magnitude_std, self.magnitude_max, increasing = 0.0, None, False
        config = config_str.split("-")
        if config[0] != "rand":
            raise ValueError(f"RandAugment: config {config_str!r} does not start with 'rand'")
        for c in config[1:]:
            cs = re.split(r"(\d.*)", c)
            if len(cs) < 2:
                continue
            key, val = cs[:2]
            if key == "mstd":
                self.magnitude_std = float(val)
                if self.magnitude_std > 100:
                    self.magnitude_std = float("inf")
            elif key == "mmax":
                self.magnitude_max = int(val)
            elif key == "inc":
                if bool(val):              # bool of the STRING, as in timm: 'inc0' is increasing too
                    increasing = True
            elif key == "m":
                self.magnitude = int(val)
            elif key == "n":
                self.num_layers = int(val)
            elif key == "p":
                self.prob = float(val)
            elif key in ("w", "t"):
                raise NotImplementedError(f"RandAugment: config key {key!r} (weighted choice / custom op list) is not implemented")
            else:
                raise ValueError(f"RandAugment: unknown config section {c!r}")
        self.names = OPS_INCREASING if increasing else OPS
        self.upper_bound = self.magnitude_max or _LEVEL_DENOM
        if 30. * self.upper_bound / _LEVEL_DENOM >= 90:
            raise ValueError(f"RandAugment: magnitudes up to {self.upper_bound} rotate by 90 degrees or more, where PIL "
                             "transposes instead of resampling; that is not implemented")
        if not served(self.batch, self.s_h, self.s_w, self.num_layers):
            raise ValueError(f"RandAugment: batch {self.batch}, {self.s_h}x{self.s_w} images, {self.num_layers} layers is outside "
                             f"the kernels' range (batch <= 4096, sides in [8, 1024], 1 to {MAX_LAYERS} layers)")
        self.plan = np.zeros((self.batch, self.num_layers, PLAN_INTS), np.int32)      # the host plan; pinned after commit()
        self.records = [[self.record("Identity")] * self.num_layers for _ in range(self.batch)]
        for k in range(self.batch):
            for l in range(self.num_layers):
                self.plan[k, l] = pack_record(self.records[k][l])
        self._device_arg = device
        self.device = None
        self._plan_pin = self._plan_dev = self._ws = self._tmp = self._event = None

    # ------------------------------------------------------------------------------------------------- host: the draw
    def level_args(self, name, magnitude):
        """timm's level functions: the op's argument at ``magnitude`` (consumes ``random.random()`` where timm negates)."""
        lv = magnitude / _LEVEL_DENOM
        if name in ("AutoContrast", "Equalize", "Invert"):
            return ()
        if name == "Rotate":
            return (_randomly_negate(lv * 30.),)
        if name in ("ShearX", "ShearY"):
            return (_randomly_negate(lv * 0.3),)
        if name in ("TranslateXRel", "TranslateYRel"):
            return (_randomly_negate(lv * 0.45),)
        if name in ("Color", "Contrast", "Brightness", "Sharpness"):
            return (lv * 1.8 + 0.1,)
        if name in ("ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing"):
            return (max(0.1, 1.0 + _randomly_negate(lv * .9)),)
        if name == "Posterize":
            return (int(lv * 4),)
        if name == "PosterizeIncreasing":
            return (4 - int(lv * 4),)
        if name == "Solarize":
            return (min(256, int(lv * 256)),)
        if name == "SolarizeIncreasing":
            return (256 - min(256, int(lv * 256)),)
        if name == "SolarizeAdd":
            return (min(128, int(lv * 110)),)
        raise ValueError(f"RandAugment: unknown op {name!r}")

    def record(self, name, *args):
        """The record of op ``name`` with timm's argument ``args`` on this image size: everything that is a pure function
        of the argument and the size is computed here, in Python, as PIL's Python layer does."""
        W, H = self.s_w, self.s_h

        def rec(kind, arg0=0, arg1=0, factor=1.0, coeffs=_IDENTITY):
            return Record(kind, int(arg0), int(arg1), float(factor), self.fill, tuple(float(v) for v in coeffs))

        base = name[:-len("Increasing")] if name.endswith("Increasing") else name
        if base == "Identity":
            return rec(K_COPY)
        if base == "AutoContrast":
            return rec(K_AUTOCONTRAST)
        if base == "Equalize":
            return rec(K_EQUALIZE)
        if base == "Invert":
            return rec(K_INVERT)
        (v,) = args
        if base == "Rotate":
            m = rotate_matrix(v, W, H)
            return rec(K_COPY) if m is None else rec(K_AFFINE, coeffs=m)
        if base == "ShearX":
            return rec(K_AFFINE, coeffs=(1, v, 0, 0, 1, 0))
        if base == "ShearY":
            return rec(K_AFFINE, coeffs=(1, 0, 0, v, 1, 0))
        if base == "TranslateXRel":
            return rec(K_AFFINE, coeffs=(1, 0, v * W, 0, 1, 0))
        if base == "TranslateYRel":
            return rec(K_AFFINE, coeffs=(1, 0, 0, 0, 1, v * H))
        if base == "Posterize":
            return rec(K_COPY) if v >= 8 else rec(K_POSTERIZE, arg0=v)      # timm returns the image at 8 bits or more
        if base == "Solarize":
            return rec(K_SOLARIZE, arg0=v)
        if base == "SolarizeAdd":
            return rec(K_SOLARIZE_ADD, arg0=v, arg1=128)
        if base in ("Color", "Contrast", "Brightness", "Sharpness"):
            return rec({"Color": K_COLOR, "Contrast": K_CONTRAST, "Brightness": K_BRIGHTNESS, "Sharpness": K_SHARPNESS}[base], factor=v)
        raise ValueError(f"RandAugment: unknown op {name!r}")

    def put(self, k, layer, rec):
        """Write ``rec`` (``record(...)``) as layer ``layer`` of sample ``k`` of the host plan."""
        if not (0 <= k < self.batch and 0 <= layer < self.num_layers):
            raise IndexError(f"RandAugment.put: sample {k}, layer {layer} of a ({self.batch}, {self.num_layers}) plan")
        if self._event is not None:                         # the last commit()'s copy still reads the pinned plan
            self._event.synchronize()
            self._event = None
        self.records[k][layer] = rec
        self.plan[k, layer] = pack_record(rec)

    def draw(self, k):
        """timm's ``RandAugment.__call__`` for sample ``k`` without the pixels: one ``np.random.choice`` over the 15 ops on
        numpy's global generator, then per layer Python's ``random`` in ``AugmentOp.__call__``'s order.  Returns the
        layers as ``(name or None if skipped, args)``."""
        if not 0 <= k < self.batch:
            raise IndexError(f"RandAugment.draw: sample {k} of a batch of {self.batch}")
        names = np.random.choice(self.names, self.num_layers, replace=True, p=None)
        drawn = []
        for layer, name in enumerate(str(n) for n in names):
            if self.prob < 1.0 and random.random() > self.prob:
                self.put(k, layer, self.record("Identity"))
                drawn.append((None, ()))
                continue
            magnitude = self.magnitude
            if self.magnitude_std > 0:
                if self.magnitude_std == float("inf"):
                    magnitude = random.uniform(0, magnitude)
                else:
                    magnitude = random.gauss(magnitude, self.magnitude_std)
            magnitude = max(0., min(magnitude, self.upper_bound))
            args = self.level_args(name, magnitude)
            self.put(k, layer, self.record(name, *args))
            drawn.append((name, args))
        return drawn

    # ------------------------------------------------------------------------------------------------------- device
    def _ensure_device(self):
        if self._plan_dev is not None:
            return
        dev = self._device_arg
        dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else torch.device(dev)
        if dev.type != "cuda":
            raise RuntimeError("fastvim_amd ops run on the GPU only (HIP kernels); RandAugment needs a GPU device")
        if not randaug_ok(self.batch, self.s_h, self.s_w, self.num_layers):
            raise ValueError("RandAugment: outside the library's range")
        self.device = dev
        self._plan_pin = torch.zeros(self.batch, self.num_layers, PLAN_INTS, dtype=torch.int32).pin_memory()
        self._plan_pin.numpy()[...] = self.plan
        self.plan = self._plan_pin.numpy()                  # draws now write pinned memory
        self._plan_dev = torch.zeros(self.batch, self.num_layers, PLAN_INTS, dtype=torch.int32, device=dev)
        n = int(L.lib().fv_randaug_workspace_bytes(L.i32(self.batch)))
        assert n == WS_BYTES * self.batch
        self._ws = torch.zeros(n, dtype=torch.uint8, device=dev)
        shape = (self.batch, 3, self.s_h, self.s_w)
        self._tmp = [torch.zeros(shape, dtype=torch.uint8, device=dev) for _ in range(min(2, self.num_layers - 1))]

    def commit(self):
        """Copy the host plan to the device (pinned memory, non-blocking, on the current stream).  The next ``draw``
        waits for that copy before it writes the host plan again."""
        self._ensure_device()
        self._plan_dev.copy_(self._plan_pin, non_blocking=True)
        if not torch.cuda.is_current_stream_capturing():
            self._event = torch.cuda.Event()
            self._event.record(torch.cuda.current_stream(self.device))

    def apply(self, src, out):
        """The launches of all layers on the plan committed last: ``src`` -> ``out``, both contiguous uint8 (batch, 3,
        S_h, S_w) on the GPU and distinct; ``src`` is left unchanged."""
        if self._plan_dev is None:
            raise RuntimeError("RandAugment.apply: nothing was committed")
        L.require_gpu(src, out)
        shape = (self.batch, 3, self.s_h, self.s_w)
        for name, t in (("src", src), ("out", out)):
            if t.dtype != torch.uint8 or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"RandAugment.apply: {name} must be a contiguous uint8 {shape} tensor, got {t.dtype} {tuple(t.shape)}")
            if t.device != self.device:
                raise RuntimeError(f"RandAugment: the plan lives on {self.device}, {name} on {t.device}")
        nbytes = src.numel()
        if src.data_ptr() < out.data_ptr() + nbytes and out.data_ptr() < src.data_ptr() + nbytes:
            raise ValueError("RandAugment.apply: src and out must be distinct buffers")
        lib, st = L.lib(), L.stream_of(out)
        b, sh, sw, nl = L.i32(self.batch), L.i32(self.s_h), L.i32(self.s_w), L.i32(self.num_layers)
        cur = src
        for layer in range(self.num_layers):
            dst = out if layer == self.num_layers - 1 else self._tmp[layer % 2]
            L.check(lib.fv_randaug_stats(L.ptr(cur), L.ptr(self._plan_dev), L.ptr(self._ws), b, sh, sw, nl, L.i32(layer), st),
                    "fv_randaug_stats")
            L.check(lib.fv_randaug_apply(L.ptr(cur), L.ptr(dst), L.ptr(self._plan_dev), L.ptr(self._ws), b, sh, sw, nl,
                                         L.i32(layer), st), "fv_randaug_apply")
            cur = dst
        return out
