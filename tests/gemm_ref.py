"""Float64 reference, per-element bounds, an fp32 emulation and the case generator for the bf16 GEMM launches behind
``fv_gemm_bf16`` and ``fv_gemm_bf16_tn_grouped(_ld)`` (csrc/gemm_mfma.hip).  CPU only: nothing here touches a GPU; the plan
queries (``fv_gemm_bf16_plan``, ``fv_gemm_bf16_tn_grouped_plan``) are host code of the library.

Reference.  ``P64 = A64 @ B64`` and ``S64 = |A64| @ |B64|`` in float64 from the bf16 operands exactly as stored (widened,
never re-rounded).

Bounds, per element; nothing is measured from the kernels.  A bf16 x bf16 product is exact in fp32 (8 + 8 significand bits),
so the only error of an fp32-accumulating GEMM is that of its K - 1 additions, each with relative error <= 2**-23 -- whichever
rounding the matrix core uses and whatever the order of summation:

* fp32 C:              ``|C - P64| <= K * 2**-23 * S64``
* ... with the (N) bias: ``+ 2**-24 * (|P64| + |bias|)`` for the one fp32 add
* bf16 C:              ``2**-8 * |P64 (+ bias)| + (1 + 2**-8) * (the fp32 bound)`` -- the half ulp of bf16 is 2**-8 relative
  (with 2**-9 a correctly rounded result reaches 1.95 x the bound)
* a split-K partial of slice s: the same over that slice's K range alone, ``K_s`` in place of K; every slice on its own.

The accumulation term is loose at long K (the emulation below sits at 1e-4 of it at K = 3072) but is the only one that holds
for an unknown summation order; sharpness at long K comes from the bit-for-bit relations of tests/test_gemm_plans_gpu.py.

Emulation (``emulate``): fp32, 64-deep K tiles accumulated in order, one rounding at the end.  tests/test_gemm_ref_cpu.py
holds it to every bound on every case and injects two faults into it (a dropped last k index, an 8-column group shifted by
one column) that the bounds must catch in every tile.

Cases.  ``gemm_cases(cus)`` / ``grouped_cases()`` ask the plan queries and state, per case, the key it reaches:
(kernel kind, A K-slow, B K-slow, fp32 C, LDS-DMA staging) for ``fv_gemm_bf16``, (tile class, LDS-DMA staging, phased form)
for one grouped launch.  The thresholds that depend on the CU count (160 x 128 tiles: a cost comparison over 2 x CUs slots;
the phased kernel: 512 tiles; the streaming kernel's trimmed tiles: more tiles than its one workgroup per CU) are searched
or computed from ``cus``, not written down.

Left out: the key (phased_tile, ...) -- the phased 256 x 256 kernel with one workgroup per tile.  It needs
``tiles <= CUs rounded down to 8`` and ``tiles >= 512`` at once, so no shape reaches it on a part with fewer than 512 CUs;
tests/test_gemm_ref_cpu.py asserts that it stays unreachable at 256 CUs, so a retune that opens it fails there.
"""
import ctypes

import torch

F64 = torch.float64
BK = 64
PAD = 1000.0          # what operand padding holds: finite, and far off if it is ever multiplied
KINDS = ("stream", "phased_tile", "phased_persistent", "wave8_256", "160x128", "128x96", "128x192", "128x128")
GROUPED_TILES = ((128, 128), (128, 192), (192, 128), (256, 256), (256, 192), (192, 256))
LEFT_OUT = ("phased_tile",)
SAMPLE_FROM = 2e10    # multiply-adds of reference from which the GPU test may check a row sample
_I = ctypes.c_int


def host_lib():
    from fastvim_amd import _lib
    return _lib.host_lib()


# ------------------------------------------------------------------------------------------------------- plan queries
def plan(M, N, K, a_ks, b_ks, c_fp32, bias, ldc, splits, cus):
    """(kind name, tile_m, tile_n, lds_dma) of the fv_gemm_bf16 launch, or None where the entry refuses the shape."""
    tm, tn, dma = _I(), _I(), _I()
    k = host_lib().fv_gemm_bf16_plan(_I(M), _I(N), _I(K), _I(a_ks), _I(b_ks), _I(c_fp32), _I(bias), _I(0), ctypes.c_long(ldc),
                                     _I(splits), _I(cus), ctypes.byref(tm), ctypes.byref(tn), ctypes.byref(dma))
    if k < 0:
        return None
    return KINDS[k], tm.value, tn.value, dma.value


def gemm_key(c, cus):
    p = plan(c["M"], c["N"], c["K"], c["a_ks"], c["b_ks"], c["c_fp32"], c["bias"], c["N"] + c["ldc_pad"], c["splits"], cus)
    return None if p is None else (p[0], c["a_ks"], c["b_ks"], c["c_fp32"], p[3])


def grouped_plan(problems):
    """problems: dicts with Kd, M, N, splits, ldx, ldy.  (tile class, lds_dma, phased) of ONE launch, or None (refused)."""
    n = len(problems)
    arr = lambda f: (_I * n)(*[p[f] for p in problems])
    dma, ph = _I(), _I()
    c = host_lib().fv_gemm_bf16_tn_grouped_plan(arr("Kd"), arr("M"), arr("N"), arr("ldx"), arr("ldy"), arr("splits"), _I(n),
                                                ctypes.byref(dma), ctypes.byref(ph))
    return None if c < 0 else (c, dma.value, ph.value)


def grouped_launches(problems):
    """The entry's cut of a problem list into balanced launches of at most 40 (include/fastvim_hip.h)."""
    launches = -(-len(problems) // 40)
    per = -(-len(problems) // launches)
    return [problems[i:i + per] for i in range(0, len(problems), per)]


# ------------------------------------------------------------------------------------------- reference and bounds
def slices(K, splits):
    kps = -(-(-(-K // splits)) // BK) * BK
    return [(k0, min(K, k0 + kps)) for k0 in range(0, K, kps)]


def reference(A64, B64, k0, k1):
    """A64 (M, K), B64 (K, N): (P64, S64) over the K range [k0, k1)."""
    a, b = A64[:, k0:k1], B64[k0:k1]
    return a @ b, a.abs() @ b.abs()


def bound(P64, S64, Ks, c_fp32, bias64=None):
    """(target, bound) per element of one slice."""
    b32 = Ks * 2.0 ** -23 * S64
    target = P64
    if bias64 is not None:
        b32 = b32 + 2.0 ** -24 * (P64.abs() + bias64.abs())
        target = P64 + bias64
    if c_fp32:
        return target, b32
    return target, 2.0 ** -8 * target.abs() + (1 + 2.0 ** -8) * b32


def ratio(C, target, bnd):
    """err / bound per element (0 / 0 = 0: an exact zero must be exact)."""
    err = (C.to(F64) - target).abs()
    r = err / bnd
    r[(err == 0) & (bnd == 0)] = 0.0
    return r


def emulate(A, B, k0, k1, c_fp32, bias=None, drop_last=False):
    """fp32 emulation: A (M, K), B (K, N) bf16 as stored; 64-deep K tiles accumulated in order; one rounding at the end."""
    a, b = A.float(), B.float()
    if drop_last:
        k1 -= 1
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32)
    for k in range(k0, k1, BK):
        acc = acc + a[:, k:min(k + BK, k1)] @ b[k:min(k + BK, k1)]
    if bias is not None:
        acc = acc + bias.float()
    return acc if c_fp32 else acc.bfloat16()


def shift_groups(C, tile_n):
    """C with the first 8-column group of every column tile shifted by one column (column j takes column j + 1; the
    group's last column takes its first): the fault of one column group written from the wrong place."""
    out = C.clone()
    N = C.shape[1]
    for n0 in range(0, N, tile_n):
        w = min(8, N - n0)
        if w >= 2:
            out[:, n0:n0 + w] = torch.roll(C[:, n0:n0 + w], -1, 1)
    return out


def tiles(M, N, tm, tn):
    for m0 in range(0, M, tm):
        for n0 in range(0, N, tn):
            yield slice(m0, min(M, m0 + tm)), slice(n0, min(N, n0 + tn))


def sample_rows(M, tile_m, seed):
    """Rows of a sampled check: first and last row of the first, second and last row tile, two seeded rows of every other
    row tile; at least 64 rows."""
    nt = -(-M // tile_m)
    g = torch.Generator().manual_seed(seed)
    rows = set()
    for t in range(nt):
        lo, hi = t * tile_m, min(M, (t + 1) * tile_m) - 1
        if t in (0, 1, nt - 1):
            rows.update((lo, hi))
        else:
            rows.update((lo + torch.randint(0, hi - lo + 1, (2,), generator=g)).tolist())
    while len(rows) < min(64, M):
        rows.add(int(torch.randint(0, M, (1,), generator=g)))
    return torch.tensor(sorted(rows))


def operands(c, seed):
    """Logical A (M, K), B (K, N) bf16 and the (N) fp32 bias of a case (CPU, seeded)."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(c["M"], c["K"], generator=g).bfloat16()
    B = torch.randn(c["K"], c["N"], generator=g).bfloat16()
    bias = torch.randn(c["N"], generator=g) if c.get("bias") else None
    return A, B, bias


def macs(c):
    return c["M"] * c["N"] * c["K"]


# ------------------------------------------------------------------------------------------------------------ cases
def _g(name, M, N, K, b=0, a=0, c32=0, bias=0, splits=1, ldc_pad=0, a_half=0, a_pad=0, b_pad=0, blocks=0):
    """a / b: K-slow flags; ldc_pad: C is a column slice of a buffer that much wider; a_half: A is the upper column half of
    a (M, 2K) buffer; a_pad / b_pad: padded operand rows; blocks: rows per block of the row-block relation (0: none)."""
    return dict(entry="gemm", name=name, M=M, N=N, K=K, a_ks=a, b_ks=b, c_fp32=c32, bias=bias, splits=splits,
                ldc_pad=ldc_pad, a_half=a_half, a_pad=a_pad, b_pad=b_pad, blocks=blocks)


def first_m(kind, lo, hi, N, K, b, c32, bias, cus):
    """Smallest M in [lo, hi) whose launch is ``kind`` (None: no such M)."""
    for M in range(lo, hi):
        p = plan(M, N, K, 0, b, c32, bias, N, 1, cus)
        if p is not None and p[0] == kind:
            return M
    return None


def gemm_cases(cus):
    """Every fv_gemm_bf16 case, each with the key it reaches at ``cus`` CUs (``key``)."""
    cs = []
    # ---- 128 x 128: every shape no other rule takes, both staging forms
    for b in (0, 1):
        nt = (4, 44, 100) if b == 0 else (8, 136)         # the element-wise tail of the 16-byte store path / narrow K-slow B
        for i, N in enumerate(nt):
            cs.append(_g(f"n{N}_b{b}", 130, N, 64, b=b, ldc_pad=8 * (i % 2), b_pad=8 * ((i + 1) % 2)))
            cs.append(_g(f"n{N}_b{b}_k40_bias", 130, N, 40, b=b, bias=1, a_half=1))     # K = 40: no DMA staging
            cs.append(_g(f"n{N}_b{b}_f32", 130, N, 128, b=b, c32=1, bias=i % 2, ldc_pad=8))
        cs.append(_g(f"k40_f32_b{b}", 130, 72, 40, b=b, c32=1, bias=1))
        cs.append(_g(f"m1_b{b}", 1, 128, 64, b=b))
        cs.append(_g(f"m8_b{b}", 8, 128, 128, b=b, bias=1))
        # 1, 2, 3, 9 and 23 tiles: remainder classes of the XCD remap; one, two and three K tiles
        for tiles_, M, N, K in ((1, 100, 128, 64), (2, 256, 128, 128), (3, 100, 320, 192), (9, 1100, 128, 192), (23, 2894, 72, 64)):
            cs.append(_g(f"t{tiles_}_b{b}", M, N, K, b=b, c32=tiles_ % 2, bias=tiles_ == 9, ldc_pad=8 * (tiles_ == 3)))
        cs.append(_g(f"k640s3_b{b}", 130, 136, 640, b=b, c32=1, splits=3, ldc_pad=8))         # short last slice
        cs.append(_g(f"k200s2_b{b}", 130, 136, 200, b=b, c32=1, splits=2))                     # ... without DMA
    for M, N, K, sp, c32 in ((8, 8, 64, 1, 1), (72, 40, 640, 3, 1), (136, 136, 200, 2, 1), (136, 264, 40, 1, 1), (264, 136, 192, 1, 0),
                             (136, 8, 40, 1, 0), (300 // 8 * 8, 128, 128, 2, 1)):
        cs.append(_g(f"tn_{M}x{N}x{K}s{sp}", M, N, K, a=1, b=1, c32=c32, splits=sp, a_pad=8 * (M > 8), b_pad=8 * (K == 640),
                     ldc_pad=8 * (K == 192)))
    # ---- 128 x 96 (N = 96, 192, 288) and 128 x 192 (N = 384, 576, ...)
    for kind_n in ((96, 192, 288), (384, 576)):
        for b in (0, 1):
            for i, N in enumerate(kind_n):
                cs.append(_g(f"n{N}_b{b}", (1, 130, 300)[i % 3], N, (64, 128, 192)[i % 3], b=b, bias=i % 2, ldc_pad=8 * (i == 1)))
                cs.append(_g(f"n{N}_b{b}_f32", (8, 260, 130)[i % 3], N, (192, 64, 128)[i % 3], b=b, c32=1, bias=(i + 1) % 2, a_half=i % 2,
                             b_pad=8 * (i == 0)))
            cs.append(_g(f"n{kind_n[-1]}_b{b}_k640s3", 130, kind_n[-1], 640, b=b, c32=1, splits=3))
            cs.append(_g(f"n{kind_n[0]}_b{b}_t23", 23 * 128 - 50, kind_n[0], 64, b=b))
    # ---- 160 x 128: where it saves a round of the 2 x CUs resident workgroups; M searched from the rule's floor
    for N, K, b, c32, bias in ((768, 192, 0, 0, 0), (768, 192, 0, 0, 1), (768, 128, 0, 1, 1), (1024, 64, 1, 0, 0), (1024, 128, 1, 0, 1),
                               (1024, 192, 1, 1, 0), (1024, 64, 0, 1, 0)):
        M = first_m("160x128", 4096, 4096 + 160 * 2 * cus, N, K, b, c32, bias, cus)
        if M is not None:
            cs.append(_g(f"m160_n{N}k{K}_b{b}{'_bias' * bias}", M, N, K, b=b, c32=c32, bias=bias, blocks=2048))
            cs.append(_g(f"m160_n{N}k{K}_b{b}{'_bias' * bias}_ragged", M + 47, N, K, b=b, c32=c32, bias=bias, ldc_pad=8, a_half=1,
                         blocks=2048))
    # ---- eight waves on 256 x 256
    cs.append(_g("w8", 4096, 2048, 512, blocks=2048))
    cs.append(_g("w8_ragged_bias", 4100, 2048, 576, bias=1, ldc_pad=8, a_half=1, b_pad=8, blocks=2048))
    cs.append(_g("w8_f32", 4100, 2048, 512, c32=1, bias=1, blocks=2048))
    cs.append(_g("w8_f32_s2", 4096, 2048, 1088, c32=1, splits=2, blocks=2048))
    # ---- streaming: every allowed N x K corner; M at the rule's floor, and with more tiles than the one workgroup per CU
    #      the launch makes (trimmed tile height, ragged last tile)
    for i, (N, K) in enumerate(((192, 768), (384, 384), (768, 192), (576, 256), (192, 128))):
        M = first_m("stream", 8192, 8192 + 4096, N, K, 1, 0, 0, cus)
        if M is None:
            continue
        cs.append(_g(f"stream_n{N}k{K}", M, N, K, b=1, bias=i % 2, blocks=2048))
        Mt = max(M, (cus // (N // 192) + 1) * 128) + 72
        cs.append(_g(f"stream_n{N}k{K}_trim", Mt, N, K, b=1, bias=(i + 1) % 2, ldc_pad=8 * (i % 2), a_half=i % 2, b_pad=8 * (i == 2),
                     blocks=2048))
    # ---- phased 256 x 256, persistent: from 512 tiles on; 7 and 9 K tiles (odd), ragged last row tile
    for name, N, K, b, ragged, ldc_pad in (("p256_k448", 2048, 448, 0, 116, 0), ("p256_k384", 2048, 384, 0, 0, 8),
                                           ("p256_k576_b1", 2048, 576, 1, 116, 0), ("p256_k512_b1", 2048, 512, 1, 0, 8)):
        M = first_m("phased_persistent", 4096, 4096 + 256 * 512, N, K, b, 0, 0, cus)
        if M is not None:
            cs.append(_g(name, (M + 255) // 256 * 256 + ragged if ragged else M, N, K, b=b, ldc_pad=ldc_pad, a_half=ragged > 0,
                         blocks=2048))
    for c in cs:
        c["key"] = gemm_key(c, cus)
        assert c["key"] is not None, c
    assert len({c["name"] for c in cs}) == len(cs)
    return cs


def _p(Kd, M, N, splits, xpad=0, ypad=0):
    return dict(Kd=Kd, M=M, N=N, splits=splits, ldx=(M + 7) // 8 * 8 + xpad, ldy=(N + 7) // 8 * 8 + ypad)


def grouped_cases():
    """Grouped launches: name, problems and the key (tile class, lds_dma, phased) of every launch the call makes."""
    cs = [
        dict(name="c0_dma", problems=[_p(640, 128, 128, 5), _p(640, 64, 40, 1), _p(1280, 136, 8, 5, xpad=8), _p(64, 8, 8, 1)]),
        dict(name="c0_regs", problems=[_p(200, 72, 40, 2), _p(40, 136, 264, 1, ypad=8)]),
        dict(name="c0_m_odd", problems=[_p(896, 44, 384, 7), _p(128, 20, 132, 1)]),            # M % 8 != 0 through ldx
        dict(name="c1_mixed_splits", problems=[_p(1792, 768, 192, 7), _p(1792, 768, 192, 4), _p(896, 384, 192, 14)]),
        dict(name="c2", problems=[_p(1792, 192, 384, 7), _p(896, 192, 768, 14, xpad=8)]),
        dict(name="c3_phased", problems=[_p(256, 512, 512, 1), _p(1792, 768, 1536, 4), _p(768, 512, 768, 3)]),
        dict(name="c3_one_k_tile", problems=[_p(64, 512, 512, 1), _p(192, 512, 768, 3), _p(640, 512, 512, 3)]),
        dict(name="c3_in_place", problems=[_p(1792, 512, 512, -1), _p(256, 512, 768, -1), _p(512, 512, 512, 2)]),
        dict(name="c4_256x192", problems=[_p(50048, 1024, 384, 46)]),
        dict(name="c5_192x256", problems=[_p(50048, 384, 768, 46)]),
        dict(name="two_launches", problems=[_p(128 + 64 * (i % 2), 64 + 8 * (i % 3), 40, 1 + i % 2) for i in range(43)]),
    ]
    for c in cs:
        c["entry"] = "grouped"
        c["keys"] = [grouped_plan(l) for l in grouped_launches(c["problems"])]
        assert None not in c["keys"], c
    return cs


# what the grouped entry documents it refuses: in-place accumulation off the phased form, a K that does not cut into whole tiles
GROUPED_REFUSED = (
    [_p(256, 192, 384, -1)],
    [_p(64, 512, 512, -1)],
    [_p(640, 128, 128, 7)],
)
