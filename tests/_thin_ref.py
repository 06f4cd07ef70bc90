"""The definition of "correct" for the one-channel-side convolutions of csrc/thin_conv.hip: a float64 reference by the formulas in that
file's header, the two families of inputs it is applied to, the bound a correct kernel has to meet on the second family, a mirror of the
host code's dispatch, and the case list shared by tests/test_thin_ref.py (CPU: proves reference and bounds on an emulation of the kernels'
arithmetic) and tests/test_thin_conv_gpu.py (the kernels themselves). Plain torch, any device, no native code.

  expand : out[n,y,x,c] = act(b[c] + sum_t s[n,y+ky-pad,x+kx-pad] * w[c,tf])          s [N][Hs][Ws] bf16, out [N][Ho][Wo][C] bf16
  squeeze: out[n,y,x]   = b + sum_t sum_c a[n,y+ky-pad,x+kx-pad,c] * w[c,tf]          a [N][Ha][Wa][C] bf16, out [N][Ho][Wo] bf16
  wgrad  : g[c,tf]      = sum_{n,y,x} a[n,y,x,c] * s[n,y+ky-pad,x+kx-pad],  asum[c] = sum a        g [C][K*K], asum [C] fp32
with t = ky*K + kx, tf = flip ? K*K-1-t : t, values outside the image zero, act = LeakyReLU(slope). Every reference also returns S, the
sum of the magnitudes of the terms of each output (|b| + sum |x * w|; sum |a * s|; sum |a| for asum).

EXACT cases. Every operand is a small multiple of 2^-2: bf16 tensors in [-3, 3], fp32 weights in [-2, 2] (about half of them zero), the
bias in [-4, 4], the slope 0.25 or 1. Every product is a multiple of 2^-4 and every partial sum, in ANY order, is a multiple of 2^-4 of
magnitude <= S; the case builder asserts S < 2^24 * 2^-4 = 2^20, so each of them is an fp32 number and no fp32 addition or fused
multiply-add rounds. Multiplying by the slope only moves the exponent. A correct kernel therefore has ONE legal result: the bf16 outputs
are the float64 reference rounded once (nearest even -- the operands produce ties), g and asum are the reference itself. The comparison
is torch.equal: no tolerance, no exclusions. These cases catch indexing mistakes: a wrong clamp, mask, flip, tap or border.

REAL-VALUED cases. randn-scaled operands with full mantissas. A kernel that accumulates in fp32 rounds every dependent operation by at
most 2^-24 of its result, and every partial result is at most S in magnitude, so a chain of D dependent roundings moves an output by at
most D * 2^-24 * S; the one rounding to bf16 adds half a bf16 ulp, 2^-8 |ref|:
    bf16 outputs: |got - ref| <= 2^-8 |ref| + D * 2^-24 * S            fp32 outputs: |got - ref| <= D * 2^-24 * S
D is read from the kernels as written (chain()):
  expand          K*K fused multiply-adds on the bias, the multiplication by the slope, one spare:                  K*K + 2
  squeeze         lane-per-channel form: K*K fma per 64-channel chunk in one accumulator, 6 butterfly steps, the bias: K*K*ceil(C/64) + 7.
                  Wide form: K*K fma per channel, 3 additions folding a thread's 8 channels, log2(C/8) <= 6 butterfly steps, the bias:
                  K*K + 10 at most, and K*K + 7 at C = 64. Both are <= K*K*ceil(C/64) + 8, which is what chain() returns.
  wgrad           one accumulator takes (rows per block) x (pixels of a row that one thread visits) fma: the wide form has 4 rows per block,
                  a thread takes 4 consecutive pixels of every (512 / C)-th quad of the row and the 64 * 8 / C pixel lanes of a channel group
                  are folded in log2(512 / C) steps; the lane-per-channel form has 2 rows per block and a thread walks the whole row in
                  steps of 2K (the masked overhang counted). The reduction kernel adds ceil(blocks / 32) partials into one of two running
                  sums (+ 1 tail), adds the two (1) and folds 16 slices serially (16): ceil(blocks / 32) + 18.
The activation is continuous (|act(u) - act(v)| <= |u - v|), so every element is compared; there is no set of borderline elements.
These cases catch precision mistakes (a truncating conversion, a bf16 accumulator); they are not asked to resolve a single dropped term.
"""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

U24, HALF_BF16 = 2.0 ** -24, 2.0 ** -8
EXACT_LIMIT = 2.0 ** 20                 # 2^24 * 2^-4
WG_ROWS, WG_ROWS_WIDE = 2, 4            # rows of `a` per block of the lane-per-channel / wide wgrad kernel (csrc/thin_conv.hip)


# ---- the host code's rules (octa_thinconv_* in csrc/thin_conv.hip), as read from it -------------------------------------------------

def shape_ok(C, K, pad, H=None, W=None):
    """shape_ok() of the host code; H, W given: the extent has to hold one window (expand, squeeze)"""
    if K not in (4, 7) or pad < 0 or pad >= K or C < 64 or C % 64 or C > 1024:
        return False
    return H is None or (H > 0 and W > 0 and H + 2 * pad >= K and W + 2 * pad >= K)


def _pow2_groups(C):
    g = C // 8
    return C % 8 == 0 and 1 <= g <= 64 and g & (g - 1) == 0


def squeeze_form(C, K):
    """'wide', 'lane' or None (refused) for octa_thinconv_squeeze"""
    if K == 3:
        return "wide" if C in (8, 16, 32, 64) else None
    if not shape_ok(C, K, 0) or C * (K * K + 1) * 4 > 64 * 1024:
        return None
    return "wide" if _pow2_groups(C) and C * K * K * 4 <= 64 * 1024 else "lane"


def wgrad_form(C, K, Wa=1):
    if not shape_ok(C, K, 0) or K * (Wa + K - 1 + 2 * K) * 4 > 60 * 1024:
        return None
    return "wide" if _pow2_groups(C) else "lane"


def expand_ok(C, K, Wo=1):
    return shape_ok(C, K, 0) and (64 * (K * K + 1) + K * (Wo + K - 1)) * 4 <= 64 * 1024


def wgrad_blocks(N, Ha, C, K):
    rows = WG_ROWS_WIDE if wgrad_form(C, K) == "wide" else WG_ROWS
    return (N * Ha + rows - 1) // rows


def chain(kind, K, C, Wa=None, blocks=None):
    """D: the longest chain of dependent fp32 roundings behind one output (module docstring)"""
    if kind == "expand":
        return K * K + 2
    if kind == "squeeze":
        return K * K * ((C + 63) // 64) + 8
    if wgrad_form(C, K) == "wide":
        qstep = 512 // C
        quads = (Wa + 3) // 4
        per_row, folds = 4 * ((quads + qstep - 1) // qstep), qstep.bit_length() - 1
        rows = WG_ROWS_WIDE
    else:
        per_row, folds, rows = 2 * K * ((Wa + 2 * K - 1) // (2 * K)), 0, WG_ROWS
    return rows * per_row + folds + (blocks + 31) // 32 + 18


# ---- the float64 reference --------------------------------------------------------------------------------------------------------------

def _window(s, Ha, Wa, K, pad):
    """s [N][Hs][Ws] -> float64 [N][Ha + K - 1][Wa + K - 1] with [n][y + ky][x + kx] = s[n][y + ky - pad][x + kx - pad], zero outside s"""
    s = s.double()
    N, Hs, Ws = s.shape
    out = s.new_zeros((N, Ha + K - 1, Wa + K - 1))
    y0, y1 = max(0, -pad), min(Hs, Ha + K - 1 - pad)
    x0, x1 = max(0, -pad), min(Ws, Wa + K - 1 - pad)
    if y1 > y0 and x1 > x0:
        out[:, y0 + pad:y1 + pad, x0 + pad:x1 + pad] = s[:, y0:y1, x0:x1]
    return out


def _tf(t, KK, flip):
    return KK - 1 - t if flip else t


def reference(kind, K, pad, flip, s=None, a=None, w=None, b=None, slope=1.0):
    """-> SimpleNamespace: expand / squeeze: out, S; wgrad: g, S_g, asum, S_asum. All float64, on the operands' device."""
    KK = K * K
    r = SimpleNamespace(kind=kind)
    if kind == "expand":
        N, Hs, Ws = s.shape
        Ho, Wo = Hs + 2 * pad - K + 1, Ws + 2 * pad - K + 1
        win, wd = _window(s, Ho, Wo, K, pad), w.double()
        C = wd.shape[0]
        bd = b.double() if b is not None else wd.new_zeros(C)
        acc = bd.expand(N, Ho, Wo, C).clone()
        r.S = bd.abs().expand(N, Ho, Wo, C).clone()
        for t in range(KK):
            term = win[:, t // K:t // K + Ho, t % K:t % K + Wo, None] * wd[:, _tf(t, KK, flip)]
            acc += term
            r.S += term.abs()
        r.out = torch.where(acc > 0, acc, acc * slope)
    elif kind == "squeeze":
        ad, wd = a.double(), w.double()
        N, Ha, Wa, C = ad.shape
        Ho, Wo = Ha + 2 * pad - K + 1, Wa + 2 * pad - K + 1
        ap = F.pad(ad, (0, 0, pad, pad, pad, pad))
        bd = b.double().reshape(()) if b is not None else ad.new_zeros(())
        r.out = bd.expand(N, Ho, Wo).clone()
        r.S = bd.abs().expand(N, Ho, Wo).clone()
        for t in range(KK):
            term = ap[:, t // K:t // K + Ho, t % K:t % K + Wo, :] * wd[:, _tf(t, KK, flip)]
            r.out += term.sum(3)
            r.S += term.abs().sum(3)
    else:
        ad = a.double()
        N, Ha, Wa, C = ad.shape
        win = _window(s, Ha, Wa, K, pad)
        r.g, r.S_g = ad.new_zeros((C, KK)), ad.new_zeros((C, KK))
        for t in range(KK):
            term = ad * win[:, t // K:t // K + Ha, t % K:t % K + Wa, None]
            r.g[:, _tf(t, KK, flip)] = term.sum((0, 1, 2))
            r.S_g[:, _tf(t, KK, flip)] = term.abs().sum((0, 1, 2))
        r.asum, r.S_asum = ad.sum((0, 1, 2)), ad.abs().sum((0, 1, 2))
    return r


def bound(ref, S, D, bf16):
    return (HALF_BF16 * ref.abs() if bf16 else 0.0) + D * U24 * S


def ratio(got, ref, S, D, bf16):
    """the largest error / bound over EVERY element; an error where the bound is 0, or a NaN, counts as inf"""
    got = got.double().reshape(ref.shape)
    err, tol = (got - ref).abs(), bound(ref, S, D, bf16)
    q = torch.where(err == 0, torch.zeros_like(err), err / tol)
    q = torch.where(torch.isnan(got), torch.full_like(q, float("inf")), q)
    return q.max().item()


def once(ref):
    """the float64 reference of an exact case rounded ONCE to bf16 (through fp32, which holds it exactly)"""
    return ref.float().to(torch.bfloat16)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
# Output extents are given; the input extent follows: Hs = Ho + K - 1 - 2 pad (expand, squeeze). For wgrad, (Ha, Wa) is the extent of `a` and
# s has Hs = Ha + K - 1 - 2 pad in BOTH roles of models/thin_conv.py (1 -> C layer: a = dy, s = x, pad, flip 0; C -> 1 layer: a = x, s = dy,
# K - 1 - pad, flip 1), so the role is the flip.

# name: (N, Ho, Wo, C, K, pad, flip, bias, slope)          Wo in {1, 3, 4, 5, 4K + 1}: waves of the block that return early, one, two quarters
EXPAND_CASES = {
    "k4_wo1": (2, 3, 1, 64, 4, 0, 0, 1, 1.0),
    "k4_wo3_ho1": (1, 1, 3, 128, 4, 1, 1, 0, 0.25),
    "k4_wo4_padmax": (2, 5, 4, 64, 4, 3, 0, 1, 0.25),
    "k4_wo5": (1, 2, 5, 128, 4, 0, 1, 1, 1.0),
    "k4_wo17": (3, 3, 17, 64, 4, 1, 1, 0, 1.0),
    "k4_wo17_padmax": (1, 6, 17, 128, 4, 3, 0, 1, 0.25),
    "k7_wo1_ho1": (2, 1, 1, 64, 7, 0, 1, 1, 0.25),
    "k7_wo3": (1, 4, 3, 128, 7, 1, 0, 0, 1.0),
    "k7_wo4": (2, 3, 4, 64, 7, 1, 0, 1, 1.0),
    "k7_wo5": (1, 2, 5, 128, 7, 0, 1, 0, 0.25),
    "k7_wo29_padmax": (2, 7, 29, 64, 7, 6, 1, 1, 1.0),
    "k7_wo29": (1, 3, 29, 128, 7, 0, 0, 1, 0.25),
    "k7_wo9_padmax": (1, 8, 9, 64, 7, 6, 0, 0, 0.25),
}

# name: (N, Ho, Wo, C, K, pad, flip, bias)
SQUEEZE_WIDE_CASES = {
    "k4_c64_wo1": (2, 3, 1, 64, 4, 0, 0, 1),
    "k4_c128_wo3_ho1": (1, 1, 3, 128, 4, 1, 1, 0),
    "k4_c256_wo4_wa1": (2, 4, 4, 256, 4, 3, 0, 1),
    "k4_c512_wo5_wa2": (1, 4, 5, 512, 4, 3, 1, 1),
    "k4_c64_wo9": (1, 2, 9, 64, 4, 1, 1, 1),
    "k4_c128_wo5_wa2": (1, 5, 5, 128, 4, 3, 0, 0),
    "k4_c512_wo9": (2, 3, 9, 512, 4, 0, 0, 0),
    "k4_c256_wo37": (1, 2, 37, 256, 4, 1, 1, 1),
    "k7_c64_wo1_ho1": (1, 1, 1, 64, 7, 0, 1, 1),
    "k7_c128_wo3": (2, 2, 3, 128, 7, 1, 0, 0),
    "k7_c256_wo9_wa3": (1, 7, 9, 256, 7, 6, 1, 1),
    "k7_c64_wo4": (1, 2, 4, 64, 7, 1, 0, 1),
    "k7_c128_wo5": (2, 2, 5, 128, 7, 0, 1, 1),
    "k7_c64_wo9": (1, 3, 9, 64, 7, 0, 0, 0),
    "k3_c8_wo1": (2, 3, 1, 8, 3, 0, 0, 1),
    "k3_c16_wo3_ho1": (1, 1, 3, 16, 3, 1, 1, 0),
    "k3_c32_wo4_wa2": (2, 4, 4, 32, 3, 2, 0, 1),
    "k3_c64_wo5": (1, 2, 5, 64, 3, 1, 1, 0),
    "k3_c8_wo9": (1, 5, 9, 8, 3, 1, 1, 0),
    "k3_c16_wo9_padmax": (1, 3, 9, 16, 3, 2, 1, 1),
}

SQUEEZE_LANE_CASES = {
    "k4_c192_wo1": (2, 3, 1, 192, 4, 0, 0, 1),
    "k4_c192_wo7": (1, 2, 7, 192, 4, 1, 1, 0),
    "k7_c192_wo8_ho1": (1, 1, 8, 192, 7, 1, 0, 1),
    "k7_c192_wo9_padmax": (1, 7, 9, 192, 7, 6, 1, 1),
    "k7_c320_wo17": (1, 2, 17, 320, 7, 0, 0, 1),
    "k4_c192_wo17_padmax": (1, 4, 17, 192, 4, 3, 1, 0),
    "k4_c960_5x6": (1, 4, 5, 960, 4, 1, 0, 1),           # a is one 5 x 6 image: 960 * 17 floats of weights fill the LDS to 256 bytes
    "k4_c960_5x6_flip": (1, 4, 5, 960, 4, 1, 1, 0),
}

# name: (N, Ha, Wa, C, K, pad, flip, asum)         blocks = ceil(N Ha / 4): the reduction's two-stream loop at 1, 15, 16, 17, 32, 33, 48, 49.
# N Ha = 189 and 195 rows need images taller than the 48 the other cases keep to: the height is the point there, the width is tiny.
WGRAD_WIDE_CASES = {
    "b1_straddle_wa1": (2, 2, 1, 64, 4, 0, 0, 1),
    "b1_wa9": (1, 3, 9, 128, 4, 2, 0, 1),
    "b15_wa2": (3, 19, 2, 128, 4, 1, 1, 0),
    "b16_wa3": (3, 21, 3, 512, 4, 1, 0, 1),
    "b17_wa4": (3, 22, 4, 64, 7, 3, 1, 1),
    "b32_wa5": (3, 42, 5, 128, 7, 0, 0, 0),
    "b33_wa9": (3, 43, 9, 512, 4, 3, 1, 1),
    "b48_wa5": (3, 63, 5, 128, 4, 3, 1, 0),
    "b49_wa1": (3, 65, 1, 64, 7, 2, 0, 1),
    "k7_c512_wa5": (2, 3, 5, 512, 7, 1, 0, 1),
    "k7_c64_wa37": (2, 5, 37, 64, 7, 1, 1, 1),           # ten quads over eight pixel lanes: two quads for some threads
    "k7_c64_ha1_pad0": (3, 1, 9, 64, 7, 0, 0, 1),        # the weight gradient of an H = K image at pad 0: a is one row high
}

# blocks = ceil(N Ha / 2), N Ha odd: the last block overhangs the last image; Ha odd: blocks straddle two images; Wa no multiple of 2K
WGRAD_LANE_CASES = {
    "k4_c192_straddle": (3, 3, 5, 192, 4, 1, 0, 1),
    "k7_c192_wa11": (1, 5, 11, 192, 7, 3, 1, 0),
    "k4_c1024_ha1": (3, 1, 9, 1024, 4, 0, 0, 1),
    "k7_c1024_padmax": (1, 7, 17, 1024, 7, 6, 1, 1),
    "k7_c192_b17_wa29": (3, 11, 29, 192, 7, 0, 0, 1),
}

FAMILIES = {"expand": EXPAND_CASES, "squeeze_wide": SQUEEZE_WIDE_CASES, "squeeze_lane": SQUEEZE_LANE_CASES,
            "wgrad_wide": WGRAD_WIDE_CASES, "wgrad_lane": WGRAD_LANE_CASES}
VARIANTS = ("exact", "real")
ALL = [(fam, name, var) for fam, cases in FAMILIES.items() for name in cases for var in VARIANTS]


def _seed(fam, name, var):
    return 1000 * sorted(FAMILIES).index(fam) + 7 * sorted(FAMILIES[fam]).index(name) + (var == "real")


def _quarters(shape, lim, gen, zero_half=False):
    """multiples of 2^-2 in [-lim, lim]"""
    v = torch.randint(-4 * lim, 4 * lim + 1, shape, generator=gen).float() / 4
    if zero_half:
        v = v * (torch.rand(shape, generator=gen) < 0.5)
    return v


def kind_of(fam):
    return fam.split("_")[0]


@functools.lru_cache(maxsize=None)
def case(fam, name, var):
    """-> SimpleNamespace(kind, K, pad, flip, slope, D, form, ops = the operands on the CPU: s / a bf16, w / b fp32 or None; want_asum).
    Drawn on the CPU from a generator seeded per case, so that the CPU proof and the GPU test see the same numbers."""
    kind = kind_of(fam)
    gen = torch.Generator().manual_seed(_seed(fam, name, var))
    exact = var == "exact"
    bf = (lambda *sh: _quarters(sh, 3, gen).to(torch.bfloat16)) if exact else (lambda *sh: torch.randn(sh, generator=gen).to(torch.bfloat16))
    c = SimpleNamespace(fam=fam, name=name, var=var, kind=kind, slope=1.0, want_asum=False)
    if kind == "wgrad":
        N, Ha, Wa, C, c.K, c.pad, c.flip, asum = FAMILIES[fam][name]
        K = c.K
        Hs, Ws = Ha + K - 1 - 2 * c.pad, Wa + K - 1 - 2 * c.pad
        assert Hs >= 1 and Ws >= 1, (fam, name)
        c.ops = dict(a=bf(N, Ha, Wa, C), s=bf(N, Hs, Ws))
        c.want_asum = bool(asum)
        c.form = wgrad_form(C, K, Wa)
        c.blocks = wgrad_blocks(N, Ha, C, K)
        c.D = chain("wgrad", K, C, Wa=Wa, blocks=c.blocks)
    else:
        spec = FAMILIES[fam][name]
        N, Ho, Wo, C, c.K, c.pad, c.flip, bias = spec[:8]
        K = c.K
        Hi, Wi = Ho + K - 1 - 2 * c.pad, Wo + K - 1 - 2 * c.pad
        assert Hi >= 1 and Wi >= 1, (fam, name)
        if kind == "expand":
            c.slope = spec[8]
            c.ops = dict(s=bf(N, Hi, Wi))
            c.form = "expand" if expand_ok(C, K, Wo) else None
        else:
            c.ops = dict(a=bf(N, Hi, Wi, C))
            c.form = squeeze_form(C, K)
        nb = C if kind == "expand" else 1
        if exact:
            c.ops["w"] = _quarters((C, K * K), 2, gen, zero_half=True)
            c.ops["b"] = _quarters((nb,), 4, gen) if bias else None
        else:
            fan = K * K * (1 if kind == "expand" else C)
            c.ops["w"] = torch.randn(C, K * K, generator=gen) / fan ** 0.5
            c.ops["b"] = torch.randn(nb, generator=gen) if bias else None
        c.D = chain(kind, K, C)
    assert c.form == {"expand": "expand", "squeeze_wide": "wide", "squeeze_lane": "lane", "wgrad_wide": "wide", "wgrad_lane": "lane"}[fam], \
        f"{fam}/{name} would not run the kernel it is listed under"
    return c


def ref_of(c, ops=None):
    """reference(...) of a case on its operands (ops: the same operands on another device); an exact case asserts its premise from S"""
    ops = c.ops if ops is None else ops
    r = reference(c.kind, c.K, c.pad, c.flip, slope=c.slope, **ops)
    if c.var == "exact":
        for S in ((r.S_g, r.S_asum) if c.kind == "wgrad" else (r.S,)):
            assert S.max().item() < EXACT_LIMIT, f"{c.fam}/{c.name}: sums reach {S.max().item()}, not exact in fp32"
    return r


@functools.lru_cache(maxsize=None)
def ref_cpu(fam, name, var):
    return ref_of(case(fam, name, var))


def outputs(c):
    """-> [(name of the output, name of its S, bf16?)]"""
    if c.kind == "wgrad":
        return [("g", "S_g", False)] + ([("asum", "S_asum", False)] if c.want_asum else [])
    return [("out", "S", True)]


def check(c, r, got, worst=None):
    """got: name -> tensor. Exact case: bit equality with the one legal result; real-valued case: every element inside its bound.
    -> name -> error / bound (0 or inf for an exact case); worst, if given, keeps the largest ratio per (kind, output)."""
    rat = {}
    for name, sname, bf16 in outputs(c):
        ref, v = getattr(r, name), got[name]
        if c.var == "exact":
            want = once(ref) if bf16 else ref.float()
            rat[name] = 0.0 if (v.dtype == want.dtype and torch.equal(v.reshape(want.shape), want)) else float("inf")
        else:
            rat[name] = ratio(v, ref, getattr(r, sname), c.D, bf16)
            if worst is not None:
                key = f"{c.fam}.{name}"
                worst[key] = max(worst.get(key, 0.0), rat[name])
    return rat
