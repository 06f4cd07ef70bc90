"""The definition of "correct" for the bf16 MFMA convolutions of csrc/conv.hip: a float64 reference by the formulas in that file, the two
families of inputs it is applied to, the bound a correct kernel has to meet on the second family, a mirror of the host code's dispatch,
and the case list shared by tests/test_conv_ref.py (CPU: proves reference and bounds on an emulation of the kernels' arithmetic) and
tests/test_conv_exact_gpu.py (the kernels themselves). Plain torch, any device, no native code. The method is that of tests/_thin_ref.py.

  forward : out[n,y,x,co] = sum_{r,s,ci} Xv[n, y*st + r - pad, x*st + s - pad, ci] * Wt[K*r + s][co][ci]       (taps of tap_mask only)
            Xv(yy, xx) = X[yy / dil][xx / dil] if 0 <= yy < H*dil, 0 <= xx < W*dil and yy, xx multiples of dil, else 0 (zero insertion);
            reflect: yy, xx are mirrored into the image first (nn.ReflectionPad2d). X = x1 | x2 on the channel axis (C1), out = y | y2 (CY1).
            s2t is the forward at st 1, dil 2, pad 1 (its header says so); fwd4 has K = 4; fwd / s2t have pad 1.
            normalise-on-load: X = bf16(lrelu(x * scale[n,c] + shift[n,c])), padding stays zero
            residual: bf16(float(bf16(acc)) + float(res)): TWO roundings
            scatter (osc, oy, ox): result pixel (y, x) is stored at (y*osc + oy, x*osc + ox) of an image osc times as large
            statistics: per (n, co) the sum and the sum of squares of the bf16-ROUNDED results; tile form float [N][tiles][Cout][2] (8 x 32
            tiles, row-major; the 16-row kernel writes this layout too), slot form double [nslot][N][Cout][2], tile t of the kernel's
            own tiling (8 or 16 rows) adds to slot t % nslot
  wgrad   : dW[K*r + s][co][ci] = sum_{n,y,x} dY[n,y,x,co] * X[n, y*st + r - pad, x*st + s - pad, ci], zero outside X (or mirrored), taps
            outside tap_mask zero; tap-major [KK][Cout][Cin] overwritten, or the parameter layout [Cout][Cin][3][3] written (SET) or
            added to (ADD). wgrad / wgrad4 have pad 1; stride 2: dY is H/2 x W/2.
Every reference also returns S, the sum of the magnitudes of the terms of each output (ADD: the buffer's own magnitude included).
Weights are drawn as nominal [KK][Cout][Cin] tensors and stored with mfma_conv.slice_major by the caller; packing is not under test.

EXACT cases. bf16 activations and gradients are multiples of 2^-2 in [-3, 3], bf16 weights multiples of 2^-2 in [-2, 2] (about half of
them zero), the residual in [-4, 4]; normalise-on-load has scale in {0.5, 1, 2}, a shift that is a multiple of 2^-2 and slope 0.25 or 1,
so every normalised value is a multiple of 2^-5 below 8: a bf16 number (asserted), and every fp32 step that makes it is exact. Products
are multiples of g = 2^-4 (2^-5, 2^-7 with normalisation at slope 1, 0.25); the builder asserts S < 2^24 g (and < 2^20), so every partial
sum in ANY order -- through the MFMA accumulation, the LDS folds, the workspace and the fp32 atomics -- is an fp32 number. A correct kernel
has ONE legal result: bf16 outputs are once(ref) (residual: the two roundings spelled out), fp32 outputs the reference itself, compared
with torch.equal. Statistics cases use integers (activations in [-2, 2], weights in {-1, 0, 1}); the sum of squares per (n, co) is
asserted below 2^24, so the tile sums, their fp32 folds and the double atomics are exact too.

REAL-VALUED cases (Cin <= 64, so that D * 2^-24 * S stays far below the bf16 half-ulp and a truncating conversion shows). Every element:
    bf16 outputs: |got - ref| <= 2^-8 |ref| + D * 2^-24 * S + E          fp32 outputs: |got - ref| <= D * 2^-24 * S + E
(residual: 2^-8 |acc| for the first rounding and 2^-8 (|acc + res| + 2^-8 |acc|) for the second).
E is the allowance of normalise-on-load: the kernel forms x * scale + shift and the slope in fp32 (three roundings at most, 2^-22 (|x scale|
+ |shift|) in all, generously) and rounds to bf16; where that fp32 error can flip the bf16 rounding the operand moves by one bf16 ulp.
normalise() returns that per-element allowance dx (zero except on such borderline elements) and E = sum |dx| |w| over the terms.
D (chain()) counts dependent fp32 roundings behind one accumulator, read from the kernels:
  forward  one accumulator takes (taps in the mask) * Cin / 16 MFMA instructions (v_mfma_f32_32x32x16_bf16: 16 products each), r roundings per
           instruction, + 1 for the fp32 addition of the residual:                                             taps * Cin / 16 * r + 1
  wgrad_tr (raw tiles, transposing reads) per tile (TW / 16) * RPW instructions per tap, RPW = TH_ / KSPLIT rows per wave, KSPLIT = 4 / PAIRS waves
           per (co, ci) pair, tiles per workgroup = ceil(n_tiles / per_block); the LDS fold of the waves sharing a pair adds KSPLIT - 1;
           then the fold of the workgroups: atomics: one rounding per arriving partial (per_block); workspace (wgrad_tr_reduce_kernel): four
           streams of ceil(per_block / 4), + 1 tail, + 2 joining them; parameter layout (wgrad_tr_acc_kernel): the same over a chunk of
           ceil(per_block / slices) partials, then `slices` atomic arrivals (or the one addition to the buffer).
  wgrad    (register-staged: scale / shift given, and the 4x4) per tile 2 * (4 / KSPLIT) instructions per tap; every wave adds its
           partial with atomics: per_block * KSPLIT arrivals.
r = R_MFMA is the number of roundings one MFMA instruction may apply to an accumulator element. r = 16: one rounding to nearest per
product, as a chain of fp32 fused multiply-adds would give; the hardware's own order inside an instruction is not documented here.

THE DISPATCH, as read from the host code (fwd_dispatch, wgrad_dispatch). The register-staged forward kernel conv3x3_nhwc_kernel<BN, ST> exists
only in its normalise-on-load form (the names reg<BN,stST,extra,masked> below), launched when scale / shift are given; every other forward call
takes the DMA-staged kernels. The register-staged weight gradient conv3x3_nhwc_wgrad_kernel exists only as xform=1,k3 (scale / shift given:
normalise-on-load compiled in) and as k4 (the 4x4 taps, without it): without scale / shift the 3x3 entry point takes the transposing-read
kernels or refuses (odd sizes at stride 2).
"""
import functools
from types import SimpleNamespace

import torch

U24, HALF_BF16 = 2.0 ** -24, 2.0 ** -8
R_MFMA = 16                              # roundings per MFMA instruction and accumulator element (module docstring)
TH, TW = 8, 32                           # output tile of the forward kernels; wgrad tiles are 4 or 8 x 32
TAP_MAJOR, PARAM_ADD, PARAM_SET = 0, 1, 2
SENT_BITS = 0x5A5B                       # the bf16 sentinel of tests/_guarded.py: what an unwritten output element holds
NUM_CUS = (256, 304)                     # the device, and a second value the dispatch is evaluated for

_DEFAULTS = dict(N=1, H=8, W=8, Cin=32, Cout=32, stride=1, dil=1, mask=None, C1=0, CY1=0, scatter=None, res=0, stats=None, norm=0, slope=1.0,
                 pad=1, reflect=0, mode=TAP_MAJOR, bias=0, real=None, fold=None, pb=None, multi=0)


def params(kind, **kw):
    p = dict(_DEFAULTS, kind=kind)
    assert set(kw) <= set(p), set(kw) - set(p)
    p.update(kw)
    p = SimpleNamespace(**p)
    p.K = 4 if kind in ("fwd4", "wgrad4") else 3
    if p.mask is None:
        p.mask = (1 << p.K * p.K) - 1
    if kind == "s2t":
        p.dil = 2
    return p


def out_extent(p):
    """(Ho, Wo) of the convolution's own result (before a scatter)"""
    if p.kind in ("wgrad", "wgrad_pad", "wgrad4"):
        if p.stride == 2:
            return p.H // 2, p.W // 2
        return p.H + 2 * p.pad - p.K + 1, p.W + 2 * p.pad - p.K + 1
    return (p.H * p.dil + 2 * p.pad - p.K) // p.stride + 1, (p.W * p.dil + 2 * p.pad - p.K) // p.stride + 1


# ---- the host code's rules, as read from it -----------------------------------------------------------------------------------------------

def fwd_refusal(p, **x):
    """why octa_conv3x3_nhwc_fwd / _fwd_pad / octa_conv3x3_s2t_nhwc / octa_conv4x4_nhwc_fwd refuse the call, or None. x: what a case never
    has: struct_size_off, both_stats, res_alias, nslot"""
    nslot = x.get("nslot", p.stats if isinstance(p.stats, int) else 0)
    slots, partials = isinstance(p.stats, int) or "nslot" in x, p.stats == "tile" or x.get("both_stats", False)
    if p.kind == "fwd" and x.get("struct_size_off"):
        return "struct_size"
    if p.N <= 0 or p.H <= 0 or p.W <= 0:
        return "bad shape"
    if p.kind == "fwd_pad":
        if slots and not 1 <= nslot <= 1024:
            return "slots"
        if p.pad < 0 or p.pad > 2 or p.H + 2 * p.pad < 3 or p.W + 2 * p.pad < 3:
            return "bad shape"
        if p.reflect and (p.pad != 1 or p.H < 2 or p.W < 2):
            return "reflection"
    if p.kind == "fwd4" and (p.pad < 0 or p.pad > 3 or p.H + 2 * p.pad < 4 or p.W + 2 * p.pad < 4):
        return "bad shape"
    if p.Cin % 32 or p.Cout % 32 or p.Cin <= 0 or p.Cout <= 0:
        return "multiples of 32"
    if p.kind == "s2t":
        return "empty tap mask or residual aliasing" if (p.mask & 0x1ff) == 0 or x.get("res_alias") else None
    if p.kind != "fwd":
        return None
    if p.stride not in (1, 2) or p.dil not in (1, 2) or (p.stride == 2 and p.dil == 2):
        return "stride / dilation"
    if (p.mask & 0x1ff) == 0:
        return "empty tap mask"
    osc, oy, ox = p.scatter or (1, 0, 0)
    if osc < 1 or osc > 2 or not 0 <= oy < osc or not 0 <= ox < osc:
        return "scatter"
    if slots and (not 1 <= nslot <= 1024 or partials or p.norm):
        return "slots"
    if (slots or partials) and (osc != 1 or p.CY1):
        return "statistics need a plain single output"
    if p.res and (osc != 1 or p.CY1 or p.norm or slots or partials or x.get("res_alias")):
        return "residual"
    C1, CY1 = p.C1 or p.Cin, p.CY1 or p.Cout
    if C1 <= 0 or C1 > p.Cin or C1 % 32 or CY1 <= 0 or CY1 > p.Cout or CY1 % 32:
        return "channel splits"
    return None


def fwd_dispatch(p):
    """-> SimpleNamespace(inst = the kernel instantiation that runs, BN, THT = rows of its tile, Ho, Wo), or None where the call is refused"""
    if fwd_refusal(p):
        return None
    Ho, Wo = out_extent(p)
    d = SimpleNamespace(Ho=Ho, Wo=Wo, THT=8)
    if p.kind == "s2t":
        d.BN, d.inst = 32, "s2t<32>"
        return d
    if p.kind == "fwd4":
        d.BN = 64 if p.Cout % 64 == 0 else 32
        d.inst = f"glds<{d.BN},st1,k4,th8>"
        return d
    stats = p.stats is not None
    if p.kind == "fwd_pad":
        d.BN = 64 if p.Cout % 64 == 0 else 32
        d.THT = 16 if d.BN == 64 and Ho >= 200 else 8
        d.inst = f"glds<{d.BN},st1,k3,th{d.THT}{',stats' if stats else ''}>"
        return d
    CY1 = p.CY1 or p.Cout
    wide = p.Cout % 64 == 0 and CY1 % 64 == 0
    d.BN = 64 if wide else 32
    osc = (p.scatter or (1, 0, 0))[0]
    masked = (p.mask & 0x1ff) != 0x1ff or osc != 1
    if p.norm:
        d.inst = f"reg<{d.BN},st{p.stride},extra,masked>"
        return d
    if p.stride == 1 and wide and not masked and Ho >= 200:
        d.THT = 16
    d.inst = f"glds<{d.BN},st{p.stride},k3,th{d.THT}{',stats' if stats else ''}{',masked' if masked else ''}>"
    return d


def fwd_instantiations():
    """every forward instantiation the entry points can launch (launch_conv_glds, launch_conv, launch_conv_s2t and their callers)"""
    s = {f"glds<{bn},st{st},k3,th8{a}{b}>" for bn in (32, 64) for st in (1, 2) for a in ("", ",stats") for b in ("", ",masked")}
    s |= {"glds<64,st1,k3,th16>", "glds<64,st1,k3,th16,stats>", "glds<32,st1,k4,th8>", "glds<64,st1,k4,th8>", "s2t<32>"}
    s |= {f"reg<{bn},st{st},extra,masked>" for bn in (32, 64) for st in (1, 2)}
    return s


def wgrad_refusal(p, **x):
    if p.kind == "wgrad" and x.get("struct_size_off"):
        return "struct_size"
    if p.mode not in (0, 1, 2):
        return "out_mode"
    if p.kind == "wgrad" and (p.mask & 0x1ff) == 0:
        return "empty tap mask"
    if p.N <= 0 or p.H <= 0 or p.W <= 0:
        return "bad shape"
    if p.kind == "wgrad4" and (p.H < 2 or p.W < 2):
        return "bad shape"
    if p.kind == "wgrad_pad":
        if p.pad < 0 or p.pad > 2 or p.H + 2 * p.pad < 3 or p.W + 2 * p.pad < 3:
            return "bad shape"
        if p.reflect and (p.pad != 1 or p.H < 2 or p.W < 2):
            return "reflection"
    if p.Cin % 32 or p.Cout % 32 or p.Cin <= 0 or p.Cout <= 0:
        return "multiples of 32"
    if p.kind != "wgrad":
        return None
    C1 = p.C1 or p.Cin
    if C1 <= 0 or C1 > p.Cin or C1 % 32:
        return "input split"
    tr = not p.norm and (p.stride == 1 or (p.stride == 2 and p.H % 2 == 0 and p.W % 2 == 0))
    if not tr:
        if p.mode:
            return "parameter layout needs the transposing-read kernels"
        if p.stride == 2 and (p.H % 2 or p.W % 2):
            return "even input sizes"
        if p.stride not in (1, 2):
            return "stride"
    return None


def wgrad_dispatch(p, num_cus):
    """-> SimpleNamespace(inst, fold = 'atomics' | 'workspace' | 'acc' | 'slices', fold_inst = the folding kernel or None, COB, CIB, TH_,
    per_block, n_tiles, tiles_per_wg, slices, KSPLIT, tr), or None where the call is refused"""
    if wgrad_refusal(p):
        return None
    Ho, Wo = out_extent(p)
    co64 = p.Cout % 64 == 0
    ci64 = p.Cin % 64 == 0 and (p.C1 or p.Cin) % 64 == 0
    d = SimpleNamespace(Ho=Ho, Wo=Wo, slices=1, fold_inst=None)
    d.tr = p.kind == "wgrad_pad" or (p.kind == "wgrad" and not p.norm)
    st = p.stride
    if p.kind == "wgrad4":
        d.COB, d.CIB = (64, 64) if co64 and p.Cin % 64 == 0 else (32, 32)
    elif st == 2:
        d.COB, d.CIB = (64, 32) if co64 else (32, 32)
    else:
        d.COB, d.CIB = 64 if co64 else 32, 64 if ci64 else 32
    pairs = (d.COB // 32) * (d.CIB // 32)
    d.KSPLIT = 4 // pairs
    blocks = (p.Cout // d.COB) * (p.Cin // d.CIB)
    two = d.COB == 32 and d.CIB == 32 and st == 1 and p.K == 3
    d.TH_ = (8 if st == 1 and d.COB == d.CIB else 4) if d.tr else 4
    d.n_tiles = ((Wo + TW - 1) // TW) * ((Ho + d.TH_ - 1) // d.TH_) * p.N
    d.per_block = max(1, min((num_cus * (2 if two else 1) + blocks - 1) // blocks, d.n_tiles))
    d.tiles_per_wg = (d.n_tiles + d.per_block - 1) // d.per_block
    if not d.tr:
        d.inst = f"wgrad<{d.COB},{d.CIB},masked={int((p.mask & 0x1ff) != 0x1ff) if p.K == 3 else 0},st{st},xform={int(bool(p.norm))},k{p.K}>"
        d.fold = "atomics"
        return d
    variant = "plain"
    if (p.mask & 0x1ff) != 0x1ff:
        variant = "tmask" if st == 2 and p.mask == 0x1b0 else "masked"
    if st == 1 and p.reflect:
        variant = "reflect"
    d.inst = f"wgrad_tr<{d.COB},{d.CIB},th{d.TH_},st{st},{variant}>"
    if p.mode:
        d.slices = min(d.per_block // 32, 16) if d.per_block > 64 else 1
        d.fold, d.fold_inst = ("slices" if d.slices > 1 else "acc"), f"acc<{d.COB},{d.CIB}>"
    elif 16 <= d.per_block <= 64:
        d.fold, d.fold_inst = "workspace", f"reduce<{d.COB},{d.CIB}>"
    else:
        d.fold = "atomics"
    return d


def wgrad_instantiations():
    s1 = ((64, 64, 8), (64, 32, 4), (32, 64, 4), (32, 32, 8))
    s = {f"wgrad_tr<{co},{ci},th{th},st1,{v}>" for co, ci, th in s1 for v in ("plain", "masked", "reflect")}
    s |= {f"wgrad_tr<{co},32,th4,st2,{v}>" for co in (64, 32) for v in ("plain", "masked", "tmask")}
    s |= {f"wgrad<{co},{ci},masked={m},st1,xform=1,k3>" for co, ci, _ in s1 for m in (0, 1)}
    s |= {f"wgrad<{co},32,masked={m},st2,xform=1,k3>" for co in (64, 32) for m in (0, 1)}
    s |= {"wgrad<64,64,masked=0,st1,xform=0,k4>", "wgrad<32,32,masked=0,st1,xform=0,k4>"}
    s |= {f"{k}<{co},{ci}>" for co, ci, _ in s1 for k in ("reduce", "acc")}
    return s


def ntaps(mask, KK):
    return bin(mask & ((1 << KK) - 1)).count("1")


def chain(p, d=None):
    """D: the longest chain of dependent fp32 roundings behind one output (module docstring); d: the wgrad dispatch"""
    if d is None:
        return ntaps(p.mask, p.K * p.K) * (p.Cin // 16) * R_MFMA + 1
    if d.tr:
        mfma = d.tiles_per_wg * (TW // 16) * (d.TH_ // d.KSPLIT)
        if d.fold == "atomics":
            fold = d.per_block
        else:
            chunk = (d.per_block + d.slices - 1) // d.slices
            fold = (chunk + 3) // 4 + 3 + (d.slices if d.fold in ("acc", "slices") else 0)
        return mfma * R_MFMA + d.KSPLIT - 1 + fold
    return d.tiles_per_wg * 2 * (4 // d.KSPLIT) * R_MFMA + d.per_block * d.KSPLIT


# ---- the float64 reference --------------------------------------------------------------------------------------------------------------

def _axis(n_out, st, off, size_v, dil, reflect, dev):
    """virtual coordinate v = i*st + off of output index i -> (source index, valid)"""
    v = torch.arange(n_out, device=dev) * st + off
    if reflect:
        v = torch.where(v < 0, -v, torch.where(v >= size_v, 2 * (size_v - 1) - v, v))
    ok = (v >= 0) & (v < size_v) & (v.clamp(min=0) % dil == 0)
    return v.clamp(0, size_v - 1) // dil, ok


def gather(x, Ho, Wo, st, dil, pad, r, s, reflect=False):
    """x [N][H][W][C] float64 -> [N][Ho][Wo][C]: Xv[n, y*st + r - pad, x*st + s - pad, :] (module docstring)"""
    N, H, W, C = x.shape
    iy, oky = _axis(Ho, st, r - pad, H * dil, dil, reflect, x.device)
    ix, okx = _axis(Wo, st, s - pad, W * dil, dil, reflect, x.device)
    return x[:, iy][:, :, ix] * (oky[:, None] & okx[None, :]).to(x.dtype)[None, :, :, None]


def conv_reference(x, w, K, st, dil, pad, reflect, mask, dx=None):
    """x [N][H][W][Cin], w [KK][Cout][Cin] float64 -> acc, S, E [N][Ho][Wo][Cout]"""
    N, H, W, _ = x.shape
    Ho, Wo = (H * dil + 2 * pad - K) // st + 1, (W * dil + 2 * pad - K) // st + 1
    acc = x.new_zeros((N, Ho, Wo, w.shape[1]))
    S, E = acc.clone(), acc.clone()
    for t in range(K * K):
        if not (mask >> t) & 1:
            continue
        g = gather(x, Ho, Wo, st, dil, pad, t // K, t % K, reflect)
        acc += torch.einsum("nyxc,oc->nyxo", g, w[t])
        S += torch.einsum("nyxc,oc->nyxo", g.abs(), w[t].abs())
        if dx is not None:
            E += torch.einsum("nyxc,oc->nyxo", gather(dx, Ho, Wo, st, dil, pad, t // K, t % K, reflect), w[t].abs())
    return acc, S, E


def wgrad_reference(x, dy, K, st, pad, reflect, mask, dx=None):
    """x [N][H][W][Cin], dy [N][Ho][Wo][Cout] float64 -> g, S, E [KK][Cout][Cin]"""
    N, Ho, Wo, Cout = dy.shape
    g = x.new_zeros((K * K, Cout, x.shape[3]))
    S, E = g.clone(), g.clone()
    for t in range(K * K):
        if not (mask >> t) & 1:
            continue
        gx = gather(x, Ho, Wo, st, 1, pad, t // K, t % K, reflect)
        g[t] = torch.einsum("nyxo,nyxc->oc", dy, gx)
        S[t] = torch.einsum("nyxo,nyxc->oc", dy.abs(), gx.abs())
        if dx is not None:
            E[t] = torch.einsum("nyxo,nyxc->oc", dy.abs(), gather(dx, Ho, Wo, st, 1, pad, t // K, t % K, reflect))
    return g, S, E


def rbf(v):
    """float64 -> the nearest bf16 number (ties to even), as float64"""
    return v.float().to(torch.bfloat16).double()


def once(ref):
    """the float64 reference of an exact case rounded ONCE to bf16 (through fp32, which holds it exactly)"""
    return ref.float().to(torch.bfloat16)


def normalise(x, scale, shift, slope):
    """x [N][H][W][C] bf16, scale / shift [N][C] fp32 -> (bf16(lrelu(x scale + shift)) as float64, dx = how far the fp32 arithmetic of a
    kernel may move that value: one bf16 ulp where its rounding is within the fp32 error of a tie, else 0, exact = no step rounded)"""
    xs = x.double() * scale.double()[:, None, None, :]
    z = xs + shift.double()[:, None, None, :]
    sl = float(torch.tensor(slope, dtype=torch.float32))
    v = torch.where(z > 0, z, z * sl)
    d = 2.0 ** -22 * (xs.abs() + shift.double().abs()[:, None, None, :])
    q = rbf(v)
    return q, (rbf(v + d) - rbf(v - d)).abs(), bool(torch.equal(q, v))


def _inputs(p, o):
    """the layer input as the kernel multiplies it: x1 | x2, normalised where scale / shift are given -> (X float64, dx or None, exact)"""
    parts, dxs, exact = [], [], True
    for i, key in ((1, "x"), (2, "x2")):
        x = o.get(key)
        if x is None:
            continue
        if o.get(f"sc{i}") is not None:
            q, d, e = normalise(x, o[f"sc{i}"], o[f"sh{i}"], p.slope)
            exact = exact and e
        else:
            q, d = x.double(), torch.zeros(x.shape, dtype=torch.float64, device=x.device)
        parts.append(q)
        dxs.append(d)
    return torch.cat(parts, 3), (torch.cat(dxs, 3) if p.norm else None), exact


def reference(p, o):
    """-> SimpleNamespace(acc, S, E [, res]) for the forward kinds, (g, S, E) in the layout of the output for the weight gradients"""
    X, dx, exact = _inputs(p, o)
    r = SimpleNamespace(norm_exact=exact)
    if p.kind in ("fwd", "fwd_pad", "s2t", "fwd4"):
        r.acc, r.S, r.E = conv_reference(X, o["w"].double(), p.K, p.stride, p.dil, p.pad, bool(p.reflect), p.mask, dx)
        r.res = o["res"].double() if p.res else None
        return r
    g, S, E = wgrad_reference(X, o["dy"].double(), p.K, p.stride, p.pad, bool(p.reflect), p.mask, dx)
    if p.mode != TAP_MAJOR:
        Co, Ci = g.shape[1], g.shape[2]
        g, S, E = (t.view(3, 3, Co, Ci).permute(2, 3, 0, 1).contiguous() for t in (g, S, E))
        if p.mode == PARAM_ADD:
            g, S = g + o["base"].double(), S + o["base"].double().abs()
    r.g, r.S, r.E = g, S, E
    return r


def stats_reference(p, d, y_rounded, nslot):
    """y_rounded [N][Ho][Wo][Cout] float64 (the bf16 results) -> the statistics buffer: nslot = 0: tile form float64 [N][tiles8][Cout][2],
    else slot form [nslot][N][Cout][2] over the tiles of the kernel's own tiling (d.THT rows)"""
    N, Ho, Wo, C = y_rounded.shape
    th = d.THT if nslot else 8
    ty, tx = (Ho + th - 1) // th, (Wo + TW - 1) // TW
    q = y_rounded.new_zeros((N, ty * th, tx * TW, C))
    q[:, :Ho, :Wo] = y_rounded
    q = q.view(N, ty, th, tx, TW, C)
    tiles = torch.stack((q.sum((2, 4)), (q * q).sum((2, 4))), -1).reshape(N, ty * tx, C, 2)
    if not nslot:
        return tiles
    slots = y_rounded.new_zeros((nslot, N, C, 2))
    for t in range(ty * tx):
        slots[t % nslot] += tiles[:, t]
    return slots


def ratio(got, ref, tol):
    """the largest error / bound over EVERY element; an error where the bound is 0, or a NaN, counts as inf"""
    got = got.double().reshape(ref.shape)
    err = (got - ref).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / tol)
    q = torch.where(torch.isnan(got), torch.full_like(q, float("inf")), q)
    return q.max().item()


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
# name: (the instantiation the case is listed under, params). Defaults: N 1, 8 x 8, 32 -> 32 channels, stride 1, all taps (_DEFAULTS).
# scatter = (2, a, b); res = residual; stats = 'tile' | nslot; norm = 1 / 2 / 3: first / second / both inputs normalised on load;
# real = False: exact variant only (Cin > 64, statistics). wgrad: mode = TAP_MAJOR / PARAM_ADD / PARAM_SET, fold = the expected fold path,
# pb = the expected per_block (both NUM_CUS), multi = a workgroup owns more than one tile.

def _fwd_cases():
    c = {}

    def add(name, inst, **kw):
        assert name not in c
        c[name] = (inst, params("fwd", **kw))

    for bn in (32, 64):
        b, g = f"bn{bn}_", f"glds<{bn},st"
        add(b + "wo1_ho1", g + "1,k3,th8>", H=1, W=1, Cout=bn)
        add(b + "wo31_ho7", g + "1,k3,th8>", H=7, W=31, Cout=bn)
        add(b + "wo32_ho8", g + "1,k3,th8>", H=8, W=32, Cout=bn)
        add(b + "wo33_ho9_n3", g + "1,k3,th8>", N=3, H=9, W=33, Cout=bn)
        add(b + "s2_odd", g + "2,k3,th8>", stride=2, H=9, W=65, Cout=bn)
        add(b + "s2_even", g + "2,k3,th8>", stride=2, H=18, W=62, Cout=bn, N=2)
        add(b + "s2_h1", g + "2,k3,th8>", stride=2, H=1, W=5, Cout=bn)
        add(b + "s2_w1", g + "2,k3,th8>", stride=2, H=4, W=1, Cout=bn)
        add(b + "dil2_h1", g + "1,k3,th8>", dil=2, H=1, W=5, Cout=bn)
        add(b + "dil2_w1", g + "1,k3,th8>", dil=2, H=5, W=1, Cout=bn)
        add(b + "dil2_wo34", g + "1,k3,th8>", dil=2, H=5, W=17, Cout=bn, Cin=64)
        add(b + "cin96", g + "1,k3,th8>", H=3, W=5, Cin=96, Cout=bn, real=False)
        add(b + "cin256", g + "1,k3,th8>", H=2, W=33, Cin=256, Cout=bn, real=False)
        add(b + "c1_32of96", g + "1,k3,th8>", H=3, W=5, Cin=96, C1=32, Cout=bn, real=False)
        add(b + "c1_64of96", g + "1,k3,th8>", H=3, W=5, Cin=96, C1=64, Cout=bn, real=False)
        add(b + "c1_96of128", g + "1,k3,th8>", H=3, W=5, Cin=128, C1=96, Cout=bn, real=False)
        add(b + "c1_32of64_s2", g + "2,k3,th8>", stride=2, H=5, W=7, Cin=64, C1=32, Cout=bn)
        add(b + "mask_centre", g + "1,k3,th8,masked>", H=5, W=33, mask=0x010, Cout=bn)
        add(b + "mask_convt", g + "1,k3,th8,masked>", dil=2, H=3, W=17, mask=0b000011011, Cout=bn)
        add(b + "mask_asym", g + "1,k3,th8,masked>", H=9, W=4, mask=0b100000110, Cout=bn)
        add(b + "mask_asym_s2", g + "2,k3,th8,masked>", stride=2, H=9, W=6, mask=0b100000110, Cout=bn)
        for a in (0, 1):
            for bb in (0, 1):
                add(b + f"scatter_{a}{bb}", g + "1,k3,th8,masked>", H=3, W=5, Cout=bn, scatter=(2, a, bb), mask=0x1ff if a == bb else 0b000011011)
        add(b + "scatter_s2_wo33", g + "2,k3,th8,masked>", stride=2, H=3, W=65, Cout=bn, scatter=(2, 1, 0))
        add(b + "res_s1", g + "1,k3,th8>", H=9, W=33, Cout=bn, res=1)
        add(b + "res_dil2", g + "1,k3,th8>", dil=2, H=3, W=17, Cout=bn, res=1)
        add(b + "res_s2_mask", g + "2,k3,th8,masked>", stride=2, H=6, W=7, mask=0x0ff, Cout=bn, res=1)
        add(b + "slot1", g + "1,k3,th8,stats>", N=2, H=9, W=33, Cout=bn, stats=1)
        add(b + "slot16", g + "1,k3,th8,stats>", N=2, H=17, W=70, Cin=64, Cout=bn, stats=16)
        add(b + "tile", g + "1,k3,th8,stats>", N=2, H=9, W=33, Cout=bn, stats="tile")
        add(b + "tile_mask", g + "1,k3,th8,stats,masked>", H=9, W=33, Cout=bn, stats="tile", mask=0x0fe)
        add(b + "slot16_s2", g + "2,k3,th8,stats>", N=2, stride=2, H=17, W=67, Cout=bn, stats=16)
        add(b + "tile_s2", g + "2,k3,th8,stats>", stride=2, H=18, W=66, Cout=bn, stats="tile")
        add(b + "slot3_s2_mask", g + "2,k3,th8,stats,masked>", stride=2, H=18, W=66, Cout=bn, stats=3, mask=0x1ef)
        add(b + "stats_large_values", g + "1,k3,th8,stats>", H=4, W=4, Cin=64, Cout=bn, stats="tile", bias=1)
        # register-staged: normalise-on-load
        r = f"reg<{bn},st"
        add(b + "norm_one", r + "1,extra,masked>", N=2, H=9, W=33, Cout=bn, norm=1, slope=0.25)
        add(b + "norm_second", r + "1,extra,masked>", N=2, H=3, W=5, Cin=64, C1=32, Cout=bn, norm=2, slope=0.25)
        add(b + "norm_first", r + "1,extra,masked>", N=2, H=3, W=5, Cin=64, C1=32, Cout=bn, norm=1, slope=1.0)
        add(b + "norm_both", r + "1,extra,masked>", N=2, H=8, W=32, Cin=64, C1=32, Cout=bn, norm=3, slope=0.25)
        add(b + "norm_s2", r + "2,extra,masked>", N=2, stride=2, H=9, W=65, Cout=bn, norm=1, slope=0.25)
        add(b + "norm_s2_even", r + "2,extra,masked>", stride=2, H=2, W=2, Cout=bn, norm=1, slope=1.0)
        add(b + "norm_dil2", r + "1,extra,masked>", dil=2, H=5, W=17, Cout=bn, norm=1, slope=0.25)
        add(b + "norm_mask", r + "1,extra,masked>", H=9, W=4, Cout=bn, norm=1, slope=0.25, mask=0b100000110)
        add(b + "norm_tile", r + "1,extra,masked>", N=2, H=3, W=33, Cout=bn, norm=1, slope=1.0, stats="tile")
        add(b + "norm_tile_s2", r + "2,extra,masked>", stride=2, H=5, W=66, Cout=bn, norm=1, slope=1.0, stats="tile")
    add("cy1_32of96", "glds<32,st1,k3,th8>", H=3, W=33, Cout=96, CY1=32)
    add("cy1_64of128", "glds<64,st1,k3,th8>", H=3, W=33, Cout=128, CY1=64)
    add("cy1_64of96", "glds<32,st1,k3,th8>", H=3, W=5, Cout=96, CY1=64)
    add("cy1_c1_s2", "glds<32,st2,k3,th8>", stride=2, H=5, W=5, Cin=64, C1=32, Cout=64, CY1=32)
    # the 16-row switch: Ho >= 200 with 64-channel blocks and all taps
    add("ho199", "glds<64,st1,k3,th8>", H=199, W=3, Cout=64)
    add("ho200", "glds<64,st1,k3,th16>", H=200, W=3, Cout=64)
    add("ho209", "glds<64,st1,k3,th16>", H=209, W=3, Cout=64)
    add("ho200_bn32", "glds<32,st1,k3,th8>", H=200, W=3, Cout=32)
    add("ho200_mask", "glds<64,st1,k3,th8,masked>", H=200, W=3, Cout=64, mask=0x1fe)
    add("ho200_dil2_res", "glds<64,st1,k3,th16>", dil=2, H=100, W=2, Cout=64, res=1)
    add("ho200_slot16", "glds<64,st1,k3,th16,stats>", H=200, W=3, Cout=64, stats=16)
    add("ho209_tile", "glds<64,st1,k3,th16,stats>", H=209, W=33, Cout=64, stats="tile")
    add("ho201_slot1", "glds<64,st1,k3,th16,stats>", H=201, W=3, Cout=64, stats=1)
    return c


def _fwd_pad_cases():
    c = {}

    def add(name, inst, **kw):
        c[name] = (inst, params("fwd_pad", **kw))

    add("pad0_3x3", "glds<32,st1,k3,th8>", H=3, W=3, pad=0)
    add("pad0_10x35", "glds<64,st1,k3,th8>", H=10, W=35, pad=0, Cout=64)
    add("pad2_1x1", "glds<64,st1,k3,th8>", H=1, W=1, pad=2, Cout=64)
    add("pad2_7x31", "glds<32,st1,k3,th8>", N=2, H=7, W=31, pad=2)
    add("reflect_2x2", "glds<32,st1,k3,th8>", H=2, W=2, reflect=1)
    add("reflect_2x33", "glds<64,st1,k3,th8>", H=2, W=33, reflect=1, Cout=64)
    add("reflect_9x8", "glds<32,st1,k3,th8>", N=2, H=9, W=8, reflect=1, Cin=64)
    add("ho199", "glds<64,st1,k3,th8>", H=199, W=3, Cout=64)
    add("ho200", "glds<64,st1,k3,th16>", H=200, W=3, Cout=64)
    add("ho200_reflect", "glds<64,st1,k3,th16>", H=200, W=2, Cout=64, reflect=1)
    add("slot16_reflect", "glds<32,st1,k3,th8,stats>", N=2, H=17, W=33, reflect=1, stats=16)
    add("slot2_bn64", "glds<64,st1,k3,th8,stats>", H=9, W=33, Cout=64, stats=2)
    add("slot16_ho200", "glds<64,st1,k3,th16,stats>", H=201, W=3, Cout=64, reflect=1, stats=16)
    return c


def _s2t_cases():
    c = {}

    def add(name, **kw):
        c[name] = ("s2t<32>", params("s2t", **kw))

    add("1x1", H=1, W=1)
    add("8x32", H=8, W=32)
    add("9x33_n2", N=2, H=9, W=33, Cout=96)
    add("convt_9x33", H=9, W=33, mask=0b000011011)
    add("convt_1x1", H=1, W=1, mask=0b000011011, Cout=96)
    add("res_9x33", H=9, W=33, res=1)
    add("res_convt_3x5", H=3, W=5, res=1, mask=0b000011011, Cout=96)
    add("cin256", H=3, W=5, Cin=256, real=False)
    add("cin256_cout96", H=2, W=33, Cin=256, Cout=96, real=False)
    return c


def _fwd4_cases():
    c = {}

    def add(name, bn, **kw):
        c[name] = (f"glds<{bn},st1,k4,th8>", params("fwd4", Cout=bn, **kw))

    for bn in (32, 64):
        add(f"bn{bn}_pad0_4x4", bn, H=4, W=4, pad=0)
        add(f"bn{bn}_pad3_1x1", bn, H=1, W=1, pad=3)
        add(f"bn{bn}_pad1_2x2", bn, H=2, W=2, pad=1)
        add(f"bn{bn}_pad1_9x34", bn, N=2, H=9, W=34, pad=1)
        add(f"bn{bn}_pad2_10x33", bn, H=10, W=33, pad=2)
    return c


_S1_FORMS = ((64, 64), (64, 32), (32, 64), (32, 32))


def _wgrad_cases():
    c = {}

    def add(name, inst, **kw):
        assert name not in c
        c[name] = (inst, params("wgrad", **kw))

    shapes = [(h, w) for h in (1, 4, 5, 8, 9) for w in (1, 31, 32, 33)]
    for co, ci in _S1_FORMS:
        th = 8 if co == ci else 4
        f, t = f"f{co}x{ci}_", f"wgrad_tr<{co},{ci},th{th},st1,"
        for i, (h, w) in enumerate(shapes):
            add(f + f"{h}x{w}", t + "plain>", N=1 + i % 2, H=h, W=w, Cout=co, Cin=ci)
        add(f + "mask", t + "masked>", N=2, H=5, W=33, Cout=co, Cin=ci, mask=0b000011011)
        add(f + "mask_set", t + "masked>", N=2, H=9, W=4, Cout=co, Cin=ci, mask=0b100000110, mode=PARAM_SET, fold="acc")
        # 16 tiles: the workspace and wgrad_tr_reduce_kernel; the same shape into the parameter layout
        add(f + "pb16", t + "plain>", N=2, H=8 * th, W=3, Cout=co, Cin=ci, pb=16, fold="workspace")
        add(f + "pb16_add", t + "plain>", N=2, H=8 * th, W=3, Cout=co, Cin=ci, pb=16, mode=PARAM_ADD, fold="acc")
        # a normalised input: the register-staged kernels (4-row tiles, atomics)
        p = f"wgrad<{co},{ci},masked="
        add(f + "norm", p + "0,st1,xform=1,k3>", N=2, H=9, W=33, Cout=co, Cin=ci, norm=1, slope=0.25)
        add(f + "norm_mask", p + "1,st1,xform=1,k3>", N=2, H=5, W=4, Cout=co, Cin=ci, norm=1, slope=1.0, mask=0b000011011)
    # a workgroup owns more than one tile (per_block = resident workgroups / channel blocks < tiles)
    add("f64x64_multi", "wgrad_tr<64,64,th8,st1,plain>", N=3, H=64, W=8, Cout=256, Cin=256, multi=1, fold="workspace", real=False)
    add("f32x32_multi", "wgrad_tr<32,32,th8,st1,plain>", N=2, H=112, W=4, Cout=160, Cin=160, C1=96, multi=1, fold="workspace", real=False)
    add("f64x32_multi", "wgrad_tr<64,32,th4,st1,plain>", N=2, H=112, W=4, Cout=128, Cin=96, multi=1, fold="workspace", real=False)
    add("f32x64_multi", "wgrad_tr<32,64,th4,st1,plain>", N=2, H=112, W=4, Cout=96, Cin=128, multi=1, fold="workspace", real=False)
    add("f32x32_norm_multi", "wgrad<32,32,masked=0,st1,xform=1,k3>", N=2, H=80, W=4, Cout=160, Cin=160, norm=1, slope=0.25, multi=1, real=False)
    # the virtual concatenation
    add("c1_32of64", "wgrad_tr<32,32,th8,st1,plain>", N=2, H=5, W=33, Cin=64, C1=32)
    add("c1_32of64_co64", "wgrad_tr<64,32,th4,st1,plain>", N=2, H=5, W=33, Cin=64, C1=32, Cout=64)
    add("c1_64of128", "wgrad_tr<64,64,th8,st1,plain>", H=9, W=5, Cin=128, C1=64, Cout=64, real=False)
    add("c1_32of64_norm2", "wgrad<32,32,masked=0,st1,xform=1,k3>", N=2, H=5, W=33, Cin=64, C1=32, norm=2, slope=0.25)
    add("c1_32of64_norm3", "wgrad<64,32,masked=0,st1,xform=1,k3>", H=4, W=9, Cin=64, C1=32, Cout=64, norm=3, slope=0.25)
    # the ways the partial sums fold: per_block = tiles (32 -> 32 channels: one channel block, 8 x 32 tiles)
    t = "wgrad_tr<32,32,th8,st1,plain>"
    for pb, (n, h, w) in ((1, (1, 8, 32)), (15, (3, 40, 3)), (16, (2, 64, 3)), (64, (2, 256, 3)), (88, (2, 176, 33))):
        for mode, mname in ((TAP_MAJOR, "tap"), (PARAM_SET, "set"), (PARAM_ADD, "add")):
            fold = ("slices" if pb > 64 else "acc") if mode else ("workspace" if 16 <= pb <= 64 else "atomics")
            add(f"pb{pb}_{mname}", t, N=n, H=h, W=w, pb=pb, mode=mode, fold=fold)
    # stride 2
    for co in (64, 32):
        f, t = f"s2_f{co}x32_", f"wgrad_tr<{co},32,th4,st2,"
        add(f + "2x2", t + "plain>", N=2, H=2, W=2, Cout=co, stride=2)
        add(f + "8x64", t + "plain>", H=8, W=64, Cout=co, stride=2)
        add(f + "10x66", t + "plain>", N=2, H=10, W=66, Cout=co, stride=2)
        add(f + "10x66_convt", t + "tmask>", N=2, H=10, W=66, Cout=co, stride=2, mask=0x1b0)
        add(f + "2x2_convt_add", t + "tmask>", H=2, W=2, Cout=co, stride=2, mask=0x1b0, mode=PARAM_ADD, fold="acc")
        add(f + "8x64_mask", t + "masked>", H=8, W=64, Cout=co, stride=2, mask=0b100000110)
        p = f"wgrad<{co},32,masked="
        add(f + "norm", p + "0,st2,xform=1,k3>", N=2, H=10, W=66, Cout=co, stride=2, norm=1, slope=0.25)
        add(f + "norm_convt", p + "1,st2,xform=1,k3>", H=2, W=2, Cout=co, stride=2, norm=1, slope=1.0, mask=0x1b0)
    return c


def _wgrad_pad_cases():
    c = {}

    def add(name, inst, **kw):
        c[name] = (inst, params("wgrad_pad", **kw))

    add("pad0_3x3", "wgrad_tr<32,32,th8,st1,plain>", N=2, H=3, W=3, pad=0)
    add("pad0_10x35_set", "wgrad_tr<64,64,th8,st1,plain>", H=10, W=35, pad=0, Cout=64, Cin=64, mode=PARAM_SET, fold="acc")
    add("pad2_1x1", "wgrad_tr<64,32,th4,st1,plain>", N=2, H=1, W=1, pad=2, Cout=64)
    add("pad2_7x31_add", "wgrad_tr<32,64,th4,st1,plain>", H=7, W=31, pad=2, Cin=64, mode=PARAM_ADD, fold="acc")
    for co, ci in _S1_FORMS:
        t = f"wgrad_tr<{co},{ci},th{8 if co == ci else 4},st1,reflect>"
        add(f"reflect_2x2_f{co}x{ci}", t, N=2, H=2, W=2, Cout=co, Cin=ci, reflect=1)
        add(f"reflect_9x33_f{co}x{ci}", t, H=9, W=33, Cout=co, Cin=ci, reflect=1, mode=(TAP_MAJOR, PARAM_ADD, PARAM_SET, TAP_MAJOR)[_S1_FORMS.index((co, ci))],
            fold=("atomics", "acc", "acc", "atomics")[_S1_FORMS.index((co, ci))])
    add("reflect_pb16", "wgrad_tr<32,32,th8,st1,reflect>", N=2, H=64, W=2, reflect=1, pb=16, fold="workspace")
    return c


def _wgrad4_cases():
    c = {}
    for ch in (64, 32):
        for n, h, w in ((2, 2, 2), (1, 5, 34), (2, 9, 9)):
            c[f"c{ch}_{h}x{w}"] = (f"wgrad<{ch},{ch},masked=0,st1,xform=0,k4>", params("wgrad4", N=n, H=h, W=w, Cin=ch, Cout=ch))
    c["c64x32_5x5"] = ("wgrad<32,32,masked=0,st1,xform=0,k4>", params("wgrad4", H=5, W=5, Cin=32, Cout=64))
    return c


FAMILIES = {"fwd": _fwd_cases(), "fwd_pad": _fwd_pad_cases(), "s2t": _s2t_cases(), "fwd4": _fwd4_cases(),
            "wgrad": _wgrad_cases(), "wgrad_pad": _wgrad_pad_cases(), "wgrad4": _wgrad4_cases()}
FORWARD = ("fwd", "fwd_pad", "s2t", "fwd4")


def has_real(p):
    return (p.Cin <= 64 and p.stats is None) if p.real is None else p.real


ALL = [(fam, name, var) for fam, cases in FAMILIES.items() for name, (_, p) in cases.items() for var in ("exact", "real") if var == "exact" or has_real(p)]


def _seed(fam, name, var):
    return 1000 * sorted(FAMILIES).index(fam) + 3 * sorted(FAMILIES[fam]).index(name) + (var == "real")


def _quarters(shape, lim, gen, zero_half=False):
    """multiples of 2^-2 in [-lim, lim]"""
    v = torch.randint(-4 * lim, 4 * lim + 1, shape, generator=gen).float() / 4
    if zero_half:
        v = v * (torch.rand(shape, generator=gen) < 0.5)
    return v


def _ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def granule(p):
    """the unit every product of an exact case is a multiple of"""
    return 2.0 ** -4 if not p.norm else (2.0 ** -5 if p.slope == 1.0 else 2.0 ** -7)


@functools.lru_cache(maxsize=None)
def case(fam, name, var, num_cus=NUM_CUS[0]):
    """-> SimpleNamespace(p, inst, d = the dispatch, D, ops = the operands on the CPU). Drawn on the CPU from a generator seeded per case, so that
    the CPU proof and the GPU test see the same numbers. Asserts that the mirror of the dispatch names the instantiation the case is listed under."""
    inst, p0 = FAMILIES[fam][name]
    p = SimpleNamespace(**vars(p0))
    if var == "real" and p.norm:
        p.slope = 0.01
    gen = torch.Generator().manual_seed(_seed(fam, name, var))
    exact, bf = var == "exact", torch.bfloat16
    c = SimpleNamespace(fam=fam, name=name, var=var, p=p)
    KK = p.K * p.K
    C1 = p.C1 or p.Cin
    if exact and p.stats is not None:
        act = lambda *sh: (_ints(sh, -2, 2, gen).abs() if p.bias else _ints(sh, -2, 2, gen)).to(bf)
    elif exact:
        act = lambda *sh: _quarters(sh, 3, gen).to(bf)
    else:
        act = lambda *sh: torch.randn(sh, generator=gen).to(bf)
    o = dict(x=act(p.N, p.H, p.W, C1), x2=act(p.N, p.H, p.W, p.Cin - C1) if p.C1 else None)
    for i, cn in ((1, C1), (2, p.Cin - C1)):
        if p.norm & i:
            if exact:
                o[f"sc{i}"] = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (p.N, cn), generator=gen)]
                o[f"sh{i}"] = _quarters((p.N, cn), 2, gen)
            else:
                o[f"sc{i}"] = 1.0 + 0.5 * torch.randn((p.N, cn), generator=gen)
                o[f"sh{i}"] = 0.5 * torch.randn((p.N, cn), generator=gen)
    Ho, Wo = out_extent(p)
    if fam in FORWARD:
        c.d = fwd_dispatch(p)
        if exact and p.stats is not None:
            w = _ints((KK, p.Cout, p.Cin), -1, 1, gen)
            if p.bias:      # output channels 0, 4, .. sum positive terms only (1, 5, ..: negative): results beyond 256, where bf16 rounds integers
                w[:, 0::4], w[:, 1::4] = w[:, 0::4].abs(), -w[:, 1::4].abs()
        elif exact:
            w = _quarters((KK, p.Cout, p.Cin), 2, gen, zero_half=True)
        else:
            w = torch.randn((KK, p.Cout, p.Cin), generator=gen) / (KK * p.Cin) ** 0.5
        for t in range(KK):         # a cleared tap is not evaluated (include/octa_hip.h): whatever its weights hold must not reach the result
            if not (p.mask >> t) & 1:
                w[t] = 1.0 if exact else 0.25
        o["w"] = w.to(bf)
        if p.res:
            o["res"] = (_quarters((p.N, Ho, Wo, p.Cout), 4, gen) if exact else torch.randn((p.N, Ho, Wo, p.Cout), generator=gen)).to(bf)
        c.D = chain(p)
    else:
        c.d = wgrad_dispatch(p, num_cus)
        o["dy"] = act(p.N, Ho, Wo, p.Cout)
        if p.mode == PARAM_ADD:
            o["base"] = _quarters((p.Cout, p.Cin, 3, 3), 8, gen) if exact else torch.randn((p.Cout, p.Cin, 3, 3), generator=gen)
        c.D = chain(p, c.d) if c.d is not None else None
    c.ops = o
    assert c.d is not None and c.d.inst == inst, f"{fam}/{name} would run {c.d and c.d.inst}, not the kernel it is listed under ({inst})"
    if fam not in FORWARD:
        assert p.fold is None or c.d.fold == p.fold, f"{fam}/{name}: fold path {c.d.fold} (per_block {c.d.per_block}), listed under {p.fold}"
        assert p.pb is None or c.d.per_block == p.pb, f"{fam}/{name}: per_block {c.d.per_block}, listed under {p.pb}"
        assert not p.multi or c.d.tiles_per_wg > 1, f"{fam}/{name}: every workgroup owns one tile only"
    return c


def ref_of(c, ops=None):
    """reference(...) of a case on its operands (ops: the same operands on another device); an exact case asserts its premise"""
    r = reference(c.p, c.ops if ops is None else ops)
    if c.var == "exact":
        lim = min(2.0 ** 20, 2.0 ** 24 * granule(c.p))
        assert r.S.max().item() < lim, f"{c.fam}/{c.name}: sums reach {r.S.max().item()}, not exact in fp32"
        assert r.norm_exact, f"{c.fam}/{c.name}: a normalised input is no bf16 number"
        if c.p.stats is not None:
            q = once(r.acc).double()
            # integers; with a normalised input (scale 0.5, shift a multiple of 2^-2, slope 1) multiples of 2^-2, squares multiples of 2^-4
            lim2 = 2.0 ** 24 * (2.0 ** -4 if c.p.norm else 1.0)
            assert (q * q).sum((1, 2)).max().item() < lim2, f"{c.fam}/{c.name}: the sum of squares reaches {(q * q).sum((1, 2)).max().item()}"
    return r


@functools.lru_cache(maxsize=None)
def ref_cpu(fam, name, var):
    return ref_of(case(fam, name, var))


def split_dense(c, dense):
    """the convolution's own result [N][Ho][Wo][Cout] -> the tensors the kernel writes: y (first CY1 channels, scattered into an image of
    sentinels where the case scatters) and y2"""
    p = c.p
    if p.scatter:
        osc, a, b = p.scatter
        N, Ho, Wo, C = dense.shape
        y = torch.full((N, Ho * osc, Wo * osc, C), SENT_BITS, dtype=torch.int16, device=dense.device).view(torch.bfloat16)
        y[:, a::osc, b::osc] = dense
        return y, None
    if p.CY1:
        return dense[..., :p.CY1].contiguous(), dense[..., p.CY1:].contiguous()
    return dense, None


def check(c, r, got, worst=None):
    """got: forward: y, y2 (None without a split), stats (None without statistics) as the kernel wrote them; wgrad: dw. Exact case: bit
    equality with the one legal result; real-valued case: every element inside its bound. -> name -> error / bound (0 or inf for an exact
    case); worst, if given, keeps the largest ratio per (family, output)."""
    p, rat = c.p, {}
    if c.fam in FORWARD:
        y = got["y"]
        if p.scatter:       # the three untouched parity classes must still hold what they held; the written one is the result
            osc, a, b = p.scatter
            keep = torch.ones(y.shape[1:3], dtype=torch.bool, device=y.device)
            keep[a::osc, b::osc] = False
            rat["untouched"] = 0.0 if bool((y.view(torch.int16)[:, keep] == SENT_BITS).all()) else float("inf")
            dense = y[:, a::osc, b::osc]
        else:
            dense = torch.cat((y, got["y2"]), 3) if p.CY1 else y
        if c.var == "exact":
            want = once(r.acc)
            if p.res:
                want = once(want.double() + r.res)
            rat["y"] = 0.0 if dense.dtype == torch.bfloat16 and dense.shape == want.shape and torch.equal(dense, want) else float("inf")
            if p.stats is not None:
                nslot = p.stats if isinstance(p.stats, int) else 0
                sw = stats_reference(p, c.d, want.double(), nslot)
                st = got["stats"]
                rat["stats"] = 0.0 if st.shape == sw.shape and torch.equal(st.double(), sw) else float("inf")
        else:
            ref = r.acc if not p.res else r.acc + r.res
            tol = HALF_BF16 * r.acc.abs() + c.D * U24 * r.S + r.E
            if p.res:
                tol = tol + HALF_BF16 * (ref.abs() + HALF_BF16 * r.acc.abs() + tol)
            rat["y"] = ratio(dense, ref, tol) if dense.shape == ref.shape else float("inf")
    else:
        dw = got["dw"]
        if c.var == "exact":
            rat["dw"] = 0.0 if dw.dtype == torch.float32 and dw.shape == r.g.shape and torch.equal(dw, r.g.float()) else float("inf")
        else:
            rat["dw"] = ratio(dw, r.g, c.D * U24 * r.S + r.E) if dw.shape == r.g.shape else float("inf")
    if worst is not None and c.var == "real":
        for k, v in rat.items():
            worst[f"{c.fam}.{k}"] = max(worst.get(f"{c.fam}.{k}", 0.0), v)
    return rat


# ---- calls the host code has to refuse (tests/test_conv_exact_gpu.py makes them with full-size buffers; tests/test_conv_ref.py asserts that
# the mirror refuses each) ---- name: (params, what a case never has) -------------------------------------------------------------------------
REFUSALS = {
    "cin_48": (params("fwd", Cin=48), {}),
    "cout_80": (params("fwd", Cout=80), {}),
    "s2_dil2": (params("fwd", stride=2, dil=2), {}),
    "stride_3": (params("fwd", stride=3), {}),
    "empty_mask": (params("fwd", mask=0x200), {}),
    "scatter_off_y": (params("fwd", scatter=(2, 2, 0)), {}),
    "scatter_off_x": (params("fwd", scatter=(1, 0, 1)), {}),
    "scatter_3": (params("fwd", scatter=(3, 0, 0)), {}),
    "c1_48": (params("fwd", Cin=96, C1=48), {}),
    "cy1_48": (params("fwd", Cout=96, CY1=48), {}),
    "stats_scatter": (params("fwd", stats="tile", scatter=(2, 0, 0)), {}),
    "slots_scatter": (params("fwd", stats=4, scatter=(2, 1, 1)), {}),
    "stats_split": (params("fwd", stats="tile", Cout=64, CY1=32), {}),
    "res_stats": (params("fwd", res=1, stats="tile"), {}),
    "res_slots": (params("fwd", res=1, stats=4), {}),
    "res_norm": (params("fwd", res=1, norm=1), {}),
    "res_scatter": (params("fwd", res=1, scatter=(2, 0, 0)), {}),
    "res_split": (params("fwd", res=1, Cout=64, CY1=32), {}),
    "res_alias": (params("fwd", res=1), dict(res_alias=True)),
    "slots_and_partials": (params("fwd", stats=4), dict(both_stats=True)),
    "slots_norm": (params("fwd", stats=4, norm=1), {}),
    "nslot_0": (params("fwd"), dict(nslot=0)),
    "nslot_1025": (params("fwd"), dict(nslot=1025)),
    "struct_size": (params("fwd"), dict(struct_size_off=True)),
    "pad_nslot_0": (params("fwd_pad"), dict(nslot=0)),
    "pad_nslot_1025": (params("fwd_pad"), dict(nslot=1025)),
    "pad_reflect_pad0": (params("fwd_pad", reflect=1, pad=0), {}),
    "pad_reflect_pad2": (params("fwd_pad", reflect=1, pad=2), {}),
    "pad_reflect_h1": (params("fwd_pad", reflect=1, H=1), {}),
    "pad_reflect_w1": (params("fwd_pad", reflect=1, W=1), {}),
    "pad_3": (params("fwd_pad", pad=3), {}),
    "pad0_2x8": (params("fwd_pad", pad=0, H=2), {}),
    "pad_cin_48": (params("fwd_pad", Cin=48), {}),
    "s2t_empty_mask": (params("s2t", mask=0), {}),
    "s2t_res_alias": (params("s2t", res=1), dict(res_alias=True)),
    "s2t_cout_48": (params("s2t", Cout=48), {}),
    "k4_pad0_3x8": (params("fwd4", pad=0, H=3), {}),
    "k4_pad1_8x1": (params("fwd4", pad=1, W=1), {}),
    "k4_pad4": (params("fwd4", pad=4), {}),
    "k4_cin_16": (params("fwd4", Cin=16), {}),
    "wgrad_cin_48": (params("wgrad", Cin=48), {}),
    "wgrad_empty_mask": (params("wgrad", mask=0), {}),
    "wgrad_c1_48": (params("wgrad", Cin=96, C1=48), {}),
    "wgrad_mode_3": (params("wgrad", mode=3), {}),
    "wgrad_s2_odd_add": (params("wgrad", stride=2, H=9, W=8, mode=PARAM_ADD), {}),
    "wgrad_s2_odd_set": (params("wgrad", stride=2, H=8, W=9, mode=PARAM_SET), {}),
    "wgrad_s2_odd": (params("wgrad", stride=2, H=9, W=9), {}),
    "wgrad_norm_add": (params("wgrad", norm=1, mode=PARAM_ADD), {}),
    "wgrad_norm_set_s2": (params("wgrad", norm=1, stride=2, mode=PARAM_SET), {}),
    "wgrad_struct_size": (params("wgrad"), dict(struct_size_off=True)),
    "wgrad_pad_reflect_pad2": (params("wgrad_pad", reflect=1, pad=2), {}),
    "wgrad_pad_reflect_h1": (params("wgrad_pad", reflect=1, H=1), {}),
    "wgrad_pad_mode_3": (params("wgrad_pad", mode=3), {}),
    "wgrad4_1x8": (params("wgrad4", H=1), {}),
    "wgrad4_cout_48": (params("wgrad4", Cout=48), {}),
}
