"""Host side of fastvim_amd.mixup.Mixup (no GPU): the numpy draw order of ``sample()`` against a restatement of
``timm.data.Mixup._params_per_batch`` / ``rand_bbox`` (timm is not a dependency: the published algorithm is restated here),
the 32-byte parameter block, the refusals, and the C ABI of the four new entry points."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest
import torch

from fastvim_amd import _lib
from fastvim_amd.mixup import Mixup, MixParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timm_params(mixup_alpha, cutmix_alpha, prob, switch_prob, correct_lam, H, W):
    """timm.data.mixup: Mixup._params_per_batch, then (in _mix_batch) the early return at lam == 1, rand_bbox and the
    lam correction -- the numpy calls in timm's order."""
    lam, use_cutmix = 1., False
    if np.random.rand() < prob:
        if mixup_alpha > 0. and cutmix_alpha > 0.:
            use_cutmix = np.random.rand() < switch_prob
            lam_mix = np.random.beta(cutmix_alpha, cutmix_alpha) if use_cutmix else np.random.beta(mixup_alpha, mixup_alpha)
        elif mixup_alpha > 0.:
            lam_mix = np.random.beta(mixup_alpha, mixup_alpha)
        elif cutmix_alpha > 0.:
            use_cutmix = True
            lam_mix = np.random.beta(cutmix_alpha, cutmix_alpha)
        else:
            lam_mix = 1.
        lam = float(lam_mix)
    if lam == 1.:
        return 1., False, (0, 0, 0, 0)
    if not use_cutmix:
        return lam, False, (0, 0, 0, 0)
    ratio = np.sqrt(1 - lam)
    cut_h, cut_w = int(H * ratio), int(W * ratio)
    cy = np.random.randint(0, H)
    cx = np.random.randint(0, W)
    yl = np.clip(cy - cut_h // 2, 0, H)
    yh = np.clip(cy + cut_h // 2, 0, H)
    xl = np.clip(cx - cut_w // 2, 0, W)
    xh = np.clip(cx + cut_w // 2, 0, W)
    if correct_lam:
        lam = 1. - (yh - yl) * (xh - xl) / float(H * W)
    return float(lam), True, (int(yl), int(yh), int(xl), int(xh))


@pytest.mark.parametrize("seed", [0, 1, 7, 1234])
@pytest.mark.parametrize("alphas", [(0.8, 1.0), (0.8, 0.0), (0.0, 1.0), (0.0, 0.0)])
@pytest.mark.parametrize("prob,correct_lam", [(1.0, True), (0.6, True), (1.0, False)])
def test_sample_follows_timms_draw_order(seed, alphas, prob, correct_lam):
    H, W = 224, 192
    n = 40
    np.random.seed(seed)
    want = [timm_params(alphas[0], alphas[1], prob, 0.5, correct_lam, H, W) for _ in range(n)]
    after_ref = np.random.rand()
    mix = Mixup(mixup_alpha=alphas[0], cutmix_alpha=alphas[1], prob=prob, switch_prob=0.5, correct_lam=correct_lam,
                label_smoothing=0.1, num_classes=1000)
    torch.manual_seed(seed)
    torch_state = torch.get_rng_state()
    np.random.seed(seed)
    got = [mix.sample((H, W)) for _ in range(n)]
    assert np.random.rand() == after_ref                       # the same NUMBER of draws, too
    assert torch.equal(torch.get_rng_state(), torch_state)     # torch's stream (DropPath's table) is left alone
    for g, w in zip(got, want):
        assert isinstance(g, MixParams) and tuple(g) == w, (g, w)
    assert mix.last() == got[-1]
    lams = [w[0] for w in want]
    if alphas == (0.0, 0.0):
        assert all(l == 1.0 for l in lams)
    else:
        assert any(l != 1.0 for l in lams)
        if prob < 1.0:
            assert any(l == 1.0 for l in lams)                 # the lam = 1 path was taken
        if alphas[1] > 0:
            assert any(w[1] for w in want)
            cut = [w for w in want if w[1]]
            assert any(b[0] == 0 or b[1] == H or b[2] == 0 or b[3] == W for _, _, b in cut)      # a box clipped at an edge
            if correct_lam:
                for lam, _, (yl, yh, xl, xh) in cut:
                    assert lam == 1. - (yh - yl) * (xh - xl) / float(H * W)


def test_zero_area_box_corrects_lam_to_one():
    """beta(a, a) close to 1 gives cut_h = cut_w = 0: an empty box, and the corrected lam is exactly 1."""
    mix = Mixup(mixup_alpha=0.0, cutmix_alpha=1.0)
    hit = 0
    for seed in range(400):
        np.random.seed(seed)
        want = timm_params(0.0, 1.0, 1.0, 0.5, True, 8, 8)
        np.random.seed(seed)
        got = mix.sample((2, 3, 8, 8))                          # a full tensor shape is accepted as well
        assert tuple(got) == want
        if got.use_cutmix and (got.box[1] - got.box[0]) * (got.box[3] - got.box[2]) == 0:
            hit += 1
            assert got.lam == 1.0
            lam32, oml32, cut = struct.unpack("<ffi", mix.packed()[:12])
            assert (lam32, oml32, cut) == (1.0, 0.0, 1)
    assert hit > 0


def test_block_layout_and_one_minus_lam_rounding():
    """struct fv_mix_params: lam, one_minus_lam (fp32), use_cutmix, yl, yh, xl, xh, reserved (int32).  one_minus_lam is the
    fp32 rounding of the DOUBLE 1 - lam -- not 1 - fp32(lam), which differs for most lam."""
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0)
    differs = 0
    np.random.seed(3)
    for _ in range(200):
        p = mix.sample((224, 224))
        b = mix.packed()
        assert len(b) == 32
        lam32, oml32, cut, yl, yh, xl, xh, rsv = struct.unpack("<ffiiiiii", b)
        assert np.float32(lam32) == np.float32(p.lam) and np.float32(oml32) == np.float32(1. - p.lam)
        assert (cut, (yl, yh, xl, xh), rsv) == (int(p.use_cutmix), p.box, 0)
        differs += np.float32(oml32) != np.float32(1) - np.float32(p.lam)
    assert differs > 0
    p = mix.set(0.3)
    assert p == MixParams(0.3, False, (0, 0, 0, 0)) and mix.last() == p
    p = mix.set(0.75, use_cutmix=True, box=(3, 9, 0, 5))
    assert struct.unpack("<ffiiiiii", mix.packed()) == (np.float32(0.75), np.float32(0.25), 1, 3, 9, 0, 5, 0)
    with pytest.raises(ValueError):
        mix.set(0.5, use_cutmix=True)
    with pytest.raises(ValueError):
        mix.set(1.5)
    hdr = open(os.path.join(ROOT, "include", "fastvim_hip.h")).read()
    m = re.search(r"typedef struct fv_mix_params \{(.*?)\} fv_mix_params;", hdr, flags=re.S)
    fields = re.findall(r"(float|int32_t)\s+([a-z_, ]+);", m.group(1))
    assert fields == [("float", "lam"), ("float", "one_minus_lam"), ("int32_t", "use_cutmix"), ("int32_t", "yl, yh, xl, xh"),
                      ("int32_t", "reserved")]


def test_cutmix_needs_an_image_size():
    mix = Mixup(mixup_alpha=0.0, cutmix_alpha=1.0)
    np.random.seed(0)
    with pytest.raises(RuntimeError, match="image size"):
        mix.sample()
    mix.bind((3, 32, 32))
    assert mix.sample().use_cutmix


@pytest.mark.parametrize("kw", [dict(mode="elem"), dict(mode="pair"), dict(cutmix_minmax=(0.2, 0.8))])
def test_unbuilt_modes_are_refused(kw):
    with pytest.raises(NotImplementedError, match="not implemented"):
        Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, **kw)


def test_odd_batch_raises():
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, num_classes=10)
    x, y = torch.zeros(3, 3, 16, 16), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match="even"):
        mix(x, y)
    with pytest.raises(ValueError, match="even"):
        mix.mix_batch(x)
    with pytest.raises(ValueError, match="even"):
        mix.criterion()(torch.zeros(3, 10), y)


def test_no_cpu_fallback():
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, num_classes=10)
    x, y = torch.zeros(4, 3, 16, 16), torch.zeros(4, dtype=torch.int64)
    from fastvim_amd.losses import CrossEntropyLoss, LabelSmoothingCrossEntropy
    for call in (lambda: mix(x, y), lambda: mix.mix_batch(x), lambda: mix.criterion()(torch.zeros(4, 10), y),
                 lambda: CrossEntropyLoss()(torch.zeros(4, 10), y), lambda: LabelSmoothingCrossEntropy(0.1)(torch.zeros(4, 10), y)):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()


def test_header_symbols_and_library_agree():
    new = ("fv_mix_batch", "fv_patch_unfold_mix", "fv_mixup_target", "fv_label_ce")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fastvim_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fv_[a-z0-9_]+)\s*\(", hdr))
    import fastvim_amd.build as fb
    fb.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in new:
        assert s in declared and s in _lib.C_ABI_SYMBOLS and hasattr(lib, s), s
    assert int(re.search(r"#define\s+FV_ABI_VERSION\s+(\d+)", hdr).group(1)) == 3 == lib.fv_version()      # additive


def test_argument_checks_need_no_gpu():
    """The entry points refuse an odd batch, too many classes and a null block before they touch the device."""
    lib = _lib.lib()
    i, p, d = ctypes.c_int, ctypes.c_void_p, ctypes.c_double
    one = p(16)                      # any non-null, 16-byte aligned value: refused calls never dereference it
    assert lib.fv_mix_batch(one, p(32), i(0), i(3), i(3), i(8), i(8), one, p(0)) == -1
    assert b"even" in lib.fv_last_error()
    assert lib.fv_mix_batch(one, p(32), i(0), i(4), i(3), i(8), i(8), p(0), p(0)) == -1
    assert lib.fv_patch_unfold_mix(one, i(0), p(32), i(1), i(5), i(3), i(16), i(16), i(8), i(8), one, p(0)) == -1
    assert b"even" in lib.fv_last_error()
    assert lib.fv_patch_unfold_mix(one, i(0), p(32), i(1), i(4), i(3), i(16), i(16), i(8), i(4), one, p(0)) == -1
    assert lib.fv_mixup_target(one, one, i(3), i(10), d(0.1), one, p(0)) == -1
    assert lib.fv_label_ce(one, i(0), one, one, d(0.1), one, one, one, p(0), p(0), i(3), i(10), p(0)) == -1
    assert b"even" in lib.fv_last_error()
    assert lib.fv_label_ce(one, i(0), one, p(0), d(0.0), one, one, one, p(0), p(0), i(3), i(4096), p(0)) == -1
    assert b"2048" in lib.fv_last_error()
