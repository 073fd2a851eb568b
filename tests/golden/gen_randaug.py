"""Writes tests/golden/randaug_pil.npz: small source images and what PIL itself computes from them for every op of timm's
RandAugment (both op lists), so that machines without PIL can hold the numpy reference (tests/randaug_ref.py) and the
kernels to PIL's bytes.  Run once with PIL installed: ``python tests/golden/gen_randaug.py``.

``pil_op(name, img, args, fill)`` is timm's op of that name (timm/data/auto_augment.py) on a PIL image, with the
``resample=BICUBIC, fillcolor=fill`` keyword arguments the reference's loaders give it; tests/test_randaug_cpu.py uses it
too.  The file holds ``src_I`` (H, W, 3) uint8; ``names`` (N,) str, ``args`` (N,) float64 (nan for ops without an
argument) and ``image`` (N,) int: case k is op ``names[k]`` at ``args[k]`` on ``src_{image[k]}``; ``out_K`` its result;
``fill`` the fill colour.

Sources: 24x40 and 37x41, each random, smooth and constant.  Arguments: timm's level functions at magnitude 9 (the recipe's
mean), 0 and 10, both signs.  The full set runs on the random 24x40 and on both constant images; the smooth images and the
random 37x41 take magnitude 9 only (their outputs do not compress)."""
import os

import numpy as np
from PIL import Image, ImageEnhance, ImageOps

FILL = (124, 116, 104)      # round(255 * IMAGENET_DEFAULT_MEAN)


def pil_op(name, img, args=(), fill=FILL):
    kw = dict(resample=Image.BICUBIC, fillcolor=tuple(fill))
    base = name[:-len("Increasing")] if name.endswith("Increasing") else name
    if base == "AutoContrast":
        return ImageOps.autocontrast(img)
    if base == "Equalize":
        return ImageOps.equalize(img)
    if base == "Invert":
        return ImageOps.invert(img)
    (v,) = args
    if base == "Rotate":
        return img.rotate(v, **kw)
    if base == "ShearX":
        return img.transform(img.size, Image.AFFINE, (1, v, 0, 0, 1, 0), **kw)
    if base == "ShearY":
        return img.transform(img.size, Image.AFFINE, (1, 0, 0, v, 1, 0), **kw)
    if base == "TranslateXRel":
        return img.transform(img.size, Image.AFFINE, (1, 0, v * img.size[0], 0, 1, 0), **kw)
    if base == "TranslateYRel":
        return img.transform(img.size, Image.AFFINE, (1, 0, 0, 0, 1, v * img.size[1]), **kw)
    if base == "Posterize":
        return img if v >= 8 else ImageOps.posterize(img, v)
    if base == "Solarize":
        return ImageOps.solarize(img, v)
    if base == "SolarizeAdd":
        lut = [min(255, i + v) if i < 128 else i for i in range(256)]
        return img.point(lut + lut + lut)
    if base == "Color":
        return ImageEnhance.Color(img).enhance(v)
    if base == "Contrast":
        return ImageEnhance.Contrast(img).enhance(v)
    if base == "Brightness":
        return ImageEnhance.Brightness(img).enhance(v)
    if base == "Sharpness":
        return ImageEnhance.Sharpness(img).enhance(v)
    raise ValueError(name)


def level_args(name, level, negate):
    """timm's level functions with the sign given instead of drawn."""
    lv, sign = level / 10., -1.0 if negate else 1.0
    if name in ("AutoContrast", "Equalize", "Invert"):
        return ()
    if name == "Rotate":
        return (sign * (lv * 30.),)
    if name in ("ShearX", "ShearY"):
        return (sign * (lv * 0.3),)
    if name in ("TranslateXRel", "TranslateYRel"):
        return (sign * (lv * 0.45),)
    if name in ("Color", "Contrast", "Brightness", "Sharpness"):
        return (lv * 1.8 + 0.1,)
    if name.endswith("Increasing") and name[:-10] in ("Color", "Contrast", "Brightness", "Sharpness"):
        return (max(0.1, 1.0 + sign * (lv * .9)),)
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
    raise ValueError(name)


NAMES = ("AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "PosterizeIncreasing", "Solarize", "SolarizeIncreasing",
         "SolarizeAdd", "Color", "ColorIncreasing", "Contrast", "ContrastIncreasing", "Brightness", "BrightnessIncreasing",
         "Sharpness", "SharpnessIncreasing", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")


def cases(levels):
    """Distinct (base op name, args) over both lists at ``levels``, both signs."""
    seen, out = set(), []
    for name in NAMES:
        for level in levels:
            for negate in (False, True):
                args = level_args(name, level, negate)
                base = name[:-len("Increasing")] if name.endswith("Increasing") else name
                key = (base, tuple(float(a) + 0.0 for a in args))      # -0.0 and 0.0 are one case
                if key not in seen:
                    seen.add(key)
                    out.append((base, args))
    return out


def smooth_image(rng, H, W):
    """A blurred random image: few distinct neighbouring values, gradients (the affine and the sharpness paths away from
    the clip)."""
    a = rng.integers(0, 256, (H + 8, W + 8, 3)).astype(np.float64)
    for _ in range(3):
        a = (a + np.roll(a, 1, 0) + np.roll(a, -1, 0) + np.roll(a, 1, 1) + np.roll(a, -1, 1)) / 5
    a = (a - a.min()) / (a.max() - a.min()) * 255
    return a[4:-4, 4:-4].round().astype(np.uint8)


def sources(rng):
    out = []
    for H, W in ((24, 40), (37, 41)):
        out.append(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
        out.append(smooth_image(rng, H, W))
        out.append(np.broadcast_to(np.array([200, 17, 90], np.uint8), (H, W, 3)).copy())
    return out      # 0 random 24x40, 1 smooth, 2 constant, 3 random 37x41, 4 smooth, 5 constant


def main():
    rng = np.random.default_rng(20241)
    srcs = sources(rng)
    out = {f"src_{i}": a for i, a in enumerate(srcs)}
    names, args, image, k = [], [], [], 0
    for i, a in enumerate(srcs):
        for name, ar in cases((9,) if i in (1, 3, 4) else (9, 0, 10)):
            img = pil_op(name, Image.fromarray(a), ar)
            names.append(name)
            args.append(float(ar[0]) if ar else float("nan"))
            image.append(i)
            out[f"out_{k}"] = np.asarray(img)
            k += 1
    out["names"], out["args"], out["image"] = np.array(names), np.array(args, np.float64), np.array(image, np.int32)
    out["fill"] = np.array(FILL, np.int32)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "randaug_pil.npz")
    np.savez_compressed(path, **out)
    print(k, "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
