"""The definition of "correct" for the fp32 MFMA convolutions of csrc/conv_f32.hip: float64 references by the formulas in that file, the two
families of inputs they are applied to, the bound a correct kernel has to meet on the second family, a mirror of the host code (dispatch,
weight-gradient plan, refusals) and the case list shared by tests/test_conv_f32_ref.py (CPU: proves reference and bounds on an emulation of
the kernels' arithmetic) and tests/test_conv_f32_exact_gpu.py (the kernels themselves). Plain torch, any device, no native code. The method
is that of tests/_conv_ref.py.

  product : out(n,co,oy,ox) = bias[co] + sum_{ci,r,s} X(n,ci, oy*S + r - pad, ox*S + s - pad) * Wp[off + (ci*K*K + r*K + s)*cout_w + co],
            X = 0 outside the image; oy < Ho, ox < Wo (given: a parity class of a data gradient reads past dy, which is zero there); the
            result is stored at (oy*osc + ooy, ox*osc + oox) of an image [Hy][Wy]; with osc = 2 every other element of that image stays as
            it was (the reference returns the mask of the written elements).
  tr      : y(n,co,2y+a,2x+b) = sum_ci x(n,ci,y,x) * Wp[(ci*4 + 2a + b)*Cout + co]      (octa_convtranspose2x2_f32_nchw, one launch)
  dgrad   : the products octa_conv2d_f32_dgrad_nchw documents, on dy and the weights in models/conv_f32.dgrad_layout:
            Conv2d stride 1: K x K, pad K - 1 - pad, taps flipped; Conv2d 3x3 stride 2 pad 1: the four parity classes (a, b), class size
            ceil((H - a) / 2) x ceil((W - b) / 2) (an empty class is skipped), (0, 0) a 1x1 product on tap slot 0 (row pitch 4 Cin), the others
            2x2 products with R(0,0) = 1, R(1,0) = 2, R(1,1) = 0 and a zero tap for (0,1), each stored scattered;
            ConvTranspose2d k = stride in {1, 2}: a k x k stride-k pad-0 product.
  wgrad   : dW[co][ci][r][s] = sum_{n,oy,ox} DY(n,co,oy,ox) * X(n,ci, oy*S + r - pad, ox*S + s - pad), db[co] = sum DY(n,co,:,:); a
            transposed layer passes its dy as X and its x as DY (dW is then its [Cin][Cout][k][k] parameter).
The forward / tr / dgrad references are DRIVEN BY THE MIRROR'S LAUNCH LIST (launches()): one product per launch the host code makes, with that
launch's sizes, padding, weight offset and row pitch. tests/test_conv_f32_ref.py proves the assembled result equal to F.conv2d /
F.conv_transpose2d / float64 autograd, so a wrong launch list fails there. Every reference also returns S, the sum of the magnitudes of the
terms of each output (bias included).

EXACT cases. Activations and gradients are multiples of 2^-2 in [-3, 3], weights multiples of 2^-2 in [-2, 2] (about half of them zero, drawn
independently per tap and channel: no symmetry a flipped or transposed tap or a swapped channel could hide behind), the bias a multiple of
2^-4 in [-2, 2]. Products are multiples of 2^-4; ref_of asserts S < 2^20, so every partial sum in ANY order -- the MFMA chain, the four-wave LDS
fold, the slab, conv_f32_wgrad_fold, conv_f32_bias_partial's threads, tree and fold -- is an fp32 number. A correct kernel has ONE legal result,
the reference itself, compared with torch.equal on the bits (unwritten elements of a scattered launch: the sentinel's bits).

REAL-VALUED cases (randn; Cin * K^2 <= 147 so that the bound stays sharp: operands rounded to 10 or 7 mantissa bits land outside it, which
tests/test_conv_f32_ref.py proves). Every element: |got - ref| <= D * 2^-24 * S.
D counts dependent fp32 roundings behind one accumulator, read from the kernels, r = 2 roundings per v_mfma_f32_32x32x2_f32 (two products):
  forward   conv_f32_kernel<K, S, MB>: slices of KC input channels (KC = 2 for K >= 7, 4 for stride 2 or K >= 4, else 8), KC / 2 instructions
            per tap and slice, channels beyond Cin multiply zeros but are issued:      D = ceil(Cin / KC) * KC * K^2 (+ 1 where a bias is added)
            (per launch: a data gradient's Cin is the layer's Cout, a parity class has K = 1 or 2)
  wgrad     conv_f32_wgrad_kernel<K, S>: a workgroup takes `rounds` = ceil(total_tiles / nchunks) tiles, a wave TH * 32 / 8 pixel pairs of
            each (TH = 8, stride 2: 2), the four waves fold in order (3), conv_f32_wgrad_fold adds nchunks partials to 0:
                                                                                         D = rounds * (TH * 4) * 2 + 3 + nchunks
  bias      conv_f32_bias_partial: per = ceil(N Ho Wo / DB_CHUNKS) values per workgroup, ceil(per / 256) per thread, a tree of 8 levels,
            conv_f32_bias_fold adds DB_CHUNKS partials:                                  D = ceil(per / 256) + 8 + DB_CHUNKS
D is derived, not fitted.

THE HOST CODE, as read from it: wide() is dispatch_f32's rule (64 channels per workgroup at stride 1 only when balance(2) >= 0.9 balance(1),
evaluated for 256 and 304 compute units), launches() the (K, S, MB, TR) instantiation and the arguments of every launch of the four entry
points, plan_wgrad() the weight-gradient plan (tiles, channel blocks, nchunks, rounds, workspace bytes), refusal() and workspace_refusal() the argument
checks of the five entry points.
"""
import functools
from types import SimpleNamespace

import torch

U24 = 2.0 ** -24
TH, TW = 8, 32
G_TARGET_WGS, DB_CHUNKS = 1024, 64
SENT_BITS = 0x5A5B5C5D                   # the fp32 sentinel of tests/_guarded.py: what an unwritten element holds
NUM_CUS = (256, 304)                     # the device, and a second value the dispatch is evaluated for
FWD_PAIRS = ((1, 1), (3, 1), (3, 2), (4, 1), (7, 1), (2, 1), (2, 2))
WGRAD_PAIRS = ((1, 1), (3, 1), (3, 2), (2, 2))
KINDS = ("fwd", "tr", "dgrad", "wgrad")

_DEFAULTS = dict(N=1, Cin=8, Cout=32, H=8, W=8, K=3, stride=1, pad=None, transposed=0, cout_w=None, w_off=0, scatter=None, bias=1, Ho=None, Wo=None,
                 real=True, ws_short=0, misalign=0)


def params(kind, **kw):
    """fwd: the arguments of octa_conv2d_f32_nchw; tr: of octa_convtranspose2x2_f32_nchw; dgrad / wgrad: the LAYER (x [N][Cin][H][W], K, stride,
    pad, transposed), as models/conv_f32.py describes it"""
    p = dict(_DEFAULTS, kind=kind)
    assert set(kw) <= set(p), set(kw) - set(p)
    p.update(kw)
    p = SimpleNamespace(**p)
    if kind == "tr":
        p.K, p.stride, p.pad, p.transposed, p.bias = 2, 2, 0, 1, 0
    if p.pad is None:
        p.pad = 0 if p.transposed else (1 if p.K == 4 else p.K // 2)
    if p.transposed:
        p.bias = 0
    eh, ew = layer_out(p)
    p.Ho, p.Wo = (eh if p.Ho is None else p.Ho), (ew if p.Wo is None else p.Wo)
    if p.cout_w is None:
        p.cout_w = p.Cout
    return p


def layer_out(p):
    if p.transposed:
        return p.H * p.K, p.W * p.K
    return (p.H + 2 * p.pad - p.K) // p.stride + 1, (p.W + 2 * p.pad - p.K) // p.stride + 1


# ---- the host code's rules, as read from it -----------------------------------------------------------------------------------------------

def kc(K, S):
    """input channels per slice of conv_f32_kernel<K, S, *>"""
    return 2 if K >= 7 else (4 if S == 2 or K >= 4 else 8)


def inst(K, S, MB, TR=False):
    return f"f32<{K},{S},{MB}{',TR' if TR else ''}>"


def fwd_instantiations():
    return {inst(K, S, MB) for K, S in FWD_PAIRS for MB in (1, 2)} | {inst(1, 1, 2, True)}


def wgrad_instantiations():
    return {f"wgrad<{K},{S}>" for K, S in WGRAD_PAIRS}


def balance(mb, N, Cout, Ho, Wo, cus):
    wgs = ((Wo + TW - 1) // TW) * ((Ho + TH - 1) // TH) * ((Cout + 32 * mb - 1) // (32 * mb)) * N
    return wgs / (cus * ((wgs + cus - 1) // cus))


def wide(N, Cout, stride, Ho, Wo, cus):
    return Cout > 32 and (stride != 1 or balance(2, N, Cout, Ho, Wo, cus) >= 0.9 * balance(1, N, Cout, Ho, Wo, cus))


def _launch(cus, N, Cin, H, W, Cout, cout_w, K, S, pad, Ho, Wo, osc=1, ooy=0, oox=0, Hy=None, Wy=None, w_off=0, bias=0):
    """one call of dispatch_f32: the product's arguments and the instantiation that runs"""
    MB = 2 if wide(N, Cout, S, Ho, Wo, cus) else 1
    return SimpleNamespace(inst=inst(K, S, MB), TR=False, MB=MB, N=N, Cin=Cin, H=H, W=W, Cout=Cout, cout_w=cout_w, K=K, S=S, pad=pad, Ho=Ho, Wo=Wo,
                           osc=osc, ooy=ooy, oox=oox, Hy=Ho * osc if Hy is None else Hy, Wy=Wo * osc if Wy is None else Wy, w_off=w_off, bias=bias,
                           D=-(-Cin // kc(K, S)) * kc(K, S) * K * K + (1 if bias else 0))


def launches(p, cus=NUM_CUS[0]):
    """every launch of conv_f32_kernel the entry point of p.kind makes, in order (fwd, tr, dgrad), or None where the call is refused"""
    if refusal(p):
        return None
    if p.kind == "fwd":
        osc, a, b = p.scatter or (1, 0, 0)
        return [_launch(cus, p.N, p.Cin, p.H, p.W, p.Cout, p.cout_w, p.K, p.stride, p.pad, p.Ho, p.Wo, osc, a, b, w_off=p.w_off, bias=p.bias)]
    if p.kind == "tr":          # one launch; M-block mb is the output column parity, blockIdx.y & 1 the row parity
        L = _launch(cus, p.N, p.Cin, p.H, p.W, p.Cout, 4 * p.Cout, 1, 1, 0, p.H, p.W, 2, 0, 0)
        L.inst, L.TR, L.MB = inst(1, 1, 2, True), True, 2
        return [L]
    assert p.kind == "dgrad"
    K, Ho, Wo = p.K, p.Ho, p.Wo
    if p.transposed and K == 2:
        return [_launch(cus, p.N, p.Cout, Ho, Wo, p.Cin, p.Cin, 2, 2, 0, p.H, p.W)]
    if p.stride == 1:
        return [_launch(cus, p.N, p.Cout, Ho, Wo, p.Cin, p.Cin, K, 1, K - 1 - p.pad, p.H, p.W)]
    out = []
    for a in (0, 1):
        for b in (0, 1):
            hp, wp, kp = (p.H - a + 1) // 2, (p.W - b + 1) // 2, (2 if (a | b) else 1)
            if hp <= 0 or wp <= 0:
                continue
            out.append(_launch(cus, p.N, p.Cout, Ho, Wo, p.Cin, 4 * p.Cin if kp == 1 else p.Cin, kp, 1, 0, hp, wp, 2, a, b, p.H, p.W,
                               w_off=(2 * a + b) * p.Cout * 4 * p.Cin))
    return out


def wgrad_operands(p):
    """the kernel's view of a weight-gradient call: (N, Cin, H, W, Cout, Ho, Wo) of its X and DY operands (a transposed layer swaps them)"""
    if p.transposed:
        return p.N, p.Cout, p.Ho, p.Wo, p.Cin, p.H, p.W
    return p.N, p.Cin, p.H, p.W, p.Cout, p.Ho, p.Wo


def plan_wgrad(N, Cin, Cout, K, stride, Ho, Wo):
    th = 8 if stride == 1 else 2
    d = SimpleNamespace(inst=f"wgrad<{K},{stride}>", TH=th, tiles_x=(Wo + TW - 1) // TW)
    d.tiles_per_img = d.tiles_x * ((Ho + th - 1) // th)
    d.total_tiles = d.tiles_per_img * N
    d.ci_blocks, d.co_blocks = (Cin + 31) // 32, (Cout + 31) // 32
    blocks = d.ci_blocks * d.co_blocks
    d.nchunks = min((G_TARGET_WGS + blocks - 1) // blocks, d.total_tiles)
    d.rounds = (d.total_tiles + d.nchunks - 1) // d.nchunks
    d.ragged = d.total_tiles % d.nchunks != 0
    d.slab_floats = d.nchunks * blocks * K * K * 1024
    d.bytes = (d.slab_floats + Cout * DB_CHUNKS) * 4
    d.D = d.rounds * (th * 4) * 2 + 3 + d.nchunks
    per = (N * Ho * Wo + DB_CHUNKS - 1) // DB_CHUNKS
    d.per, d.D_bias = per, (per + 255) // 256 + 8 + DB_CHUNKS
    return d


def wgrad_dispatch(p):
    if refusal(p):
        return None
    N, Cin, _, _, Cout, Ho, Wo = wgrad_operands(p)
    return plan_wgrad(N, Cin, Cout, p.K, p.stride, Ho, Wo)


def _beyond(p, H, W, Ho, Wo):
    return (Ho - 1) * p.stride + p.K - p.pad > H + p.pad or (Wo - 1) * p.stride + p.K - p.pad > W + p.pad


def refusal(p):
    """the text the entry point of p.kind puts into its error message when it refuses the call (a part of it), or None"""
    pos = all(v > 0 for v in (p.N, p.Cin, p.H, p.W, p.Cout, p.Ho, p.Wo)) and p.pad >= 0
    if p.kind == "fwd":
        if not pos or p.cout_w < p.Cout:
            return "bad arguments"
        osc, a, b = p.scatter or (1, 0, 0)
        if osc not in (1, 2) or not 0 <= a < osc or not 0 <= b < osc:
            return "bad output scatter"
        if _beyond(p, p.H, p.W, p.Ho, p.Wo):
            return "reads beyond the padded input"
        if p.Cin * p.H * p.W >= 2 ** 31:
            return "exceeds 2^31 elements"
        return None if (p.K, p.stride) in FWD_PAIRS else "is not instantiated"
    if p.kind == "tr":
        if not pos:
            return "bad arguments"
        if p.Cin * p.H * p.W >= 2 ** 31:
            return "exceeds 2^31 elements"
        return "the output must be 8-byte aligned" if p.misalign else None
    if p.kind == "dgrad":
        if not pos:
            return "bad arguments"
        ok = (p.K in (1, 2) and p.stride == p.K and p.pad == 0) if p.transposed else (p.K, p.stride, p.pad) in ((1, 1, 0), (3, 1, 1), (3, 2, 1))
        if not ok:
            return "is not covered"
        if (p.Ho, p.Wo) != layer_out(p):
            return "the layer gives"
        return "exceeds 2^31 elements" if p.Cout * p.Ho * p.Wo >= 2 ** 31 or p.Cin * p.H * p.W >= 2 ** 31 else None
    assert p.kind == "wgrad"
    N, Cin, H, W, Cout, Ho, Wo = wgrad_operands(p)
    if not pos or p.pad >= p.K:
        return "bad arguments"
    if _beyond(p, H, W, Ho, Wo):
        return "reads beyond the padded input"
    if Cin * H * W >= 2 ** 31 or Cout * Ho * Wo >= 2 ** 31:
        return "exceeds 2^31 elements"
    if p.ws_short:
        return "needed"
    return None if (p.K, p.stride) in WGRAD_PAIRS else "is not instantiated"


def workspace_refusal(N, Cin, H, W, Cout, K, stride, pad, Ho, Wo):
    """octa_conv2d_f32_wgrad_workspace answers any positive shape (it plans; octa_conv2d_f32_wgrad_nchw judges K / stride and the extents)"""
    return None if min(N, Cin, H, W, Cout, K, stride, Ho, Wo) > 0 and pad >= 0 else "bad arguments"


# ---- the float64 reference --------------------------------------------------------------------------------------------------------------

def _axis(n_out, st, off, size, dev):
    v = torch.arange(n_out, device=dev) * st + off
    return v.clamp(0, size - 1), (v >= 0) & (v < size)


def gather(x, Ho, Wo, st, pad, r, s):
    """x [N][C][H][W] -> [N][C][Ho][Wo]: X(n, c, oy*st + r - pad, ox*st + s - pad), zero outside the image"""
    iy, oky = _axis(Ho, st, r - pad, x.shape[2], x.device)
    ix, okx = _axis(Wo, st, s - pad, x.shape[3], x.device)
    return x[:, :, iy][:, :, :, ix] * (oky[:, None] & okx[None, :]).to(x.dtype)


def weights_of(wflat, L, KK=None):
    """the weights one launch reads, [Cin][K*K][Cout], from the flat packed buffer: element off + (ci*K*K + t)*cout_w + co"""
    KK = L.K * L.K if KK is None else KK
    idx = L.w_off + (torch.arange(L.Cin * KK, device=wflat.device)[:, None] * L.cout_w + torch.arange(L.Cout, device=wflat.device)[None, :])
    return wflat[idx].view(L.Cin, KK, L.Cout)


def product(x, wflat, L, bias=None):
    """one launch -> (acc, S) [N][Cout][Ho][Wo] float64"""
    x, w = x.double(), weights_of(wflat.double(), L)
    acc = x.new_zeros((L.N, L.Cout, L.Ho, L.Wo))
    S = acc.clone()
    for t in range(L.K * L.K):
        g = gather(x, L.Ho, L.Wo, L.S, L.pad, t // L.K, t % L.K)
        acc += torch.einsum("nchw,co->nohw", g, w[:, t])
        S += torch.einsum("nchw,co->nohw", g.abs(), w[:, t].abs())
    if bias is not None:
        acc, S = acc + bias.double()[None, :, None, None], S + bias.double().abs()[None, :, None, None]
    return acc, S


def assemble(x, wflat, Ls, bias=None):
    """the launches of one entry-point call -> SimpleNamespace(ref, S, D [N][Cout][Hy][Wy] float64, written [Hy][Wy] bool)"""
    L0 = Ls[0]
    r = SimpleNamespace(ref=torch.zeros((L0.N, L0.Cout, L0.Hy, L0.Wy), dtype=torch.float64, device=x.device))
    r.S, r.D = r.ref.clone(), r.ref.clone()
    r.written = torch.zeros((L0.Hy, L0.Wy), dtype=torch.bool, device=x.device)
    for L in Ls:
        if L.TR:        # Wp [Cin][tap 2a + b][Cout]: the 1x1 product of tap 2a + b goes to parity (a, b)
            for a in (0, 1):
                for b in (0, 1):
                    Lt = SimpleNamespace(**dict(vars(L), w_off=(2 * a + b) * L.Cout))
                    acc, S = product(x, wflat, Lt)
                    r.ref[:, :, a::2, b::2], r.S[:, :, a::2, b::2] = acc, S
            r.D[:], r.written[:] = L.D, True
            continue
        acc, S = product(x, wflat, L, bias if L.bias else None)
        sl = (slice(None), slice(None), slice(L.ooy, None, L.osc), slice(L.oox, None, L.osc))
        assert not bool(r.written[sl[2:]][:L.Ho, :L.Wo].any()), "two launches write one element"
        r.ref[sl][:, :, :L.Ho, :L.Wo], r.S[sl][:, :, :L.Ho, :L.Wo], r.D[sl][:, :, :L.Ho, :L.Wo] = acc, S, L.D
        r.written[sl[2:]][:L.Ho, :L.Wo] = True
    return r


def wgrad_reference(x, dy, K, st, pad):
    """kernel operands x [N][Cin][H][W], dy [N][Cout][Ho][Wo] -> g, Sg [Cout][Cin][K][K], db, Sdb [Cout] float64"""
    x, dy = x.double(), dy.double()
    Ho, Wo = dy.shape[2], dy.shape[3]
    g = x.new_zeros((dy.shape[1], x.shape[1], K, K))
    S = g.clone()
    for t in range(K * K):
        gx = gather(x, Ho, Wo, st, pad, t // K, t % K)
        g[:, :, t // K, t % K] = torch.einsum("nohw,nchw->oc", dy, gx)
        S[:, :, t // K, t % K] = torch.einsum("nohw,nchw->oc", dy.abs(), gx.abs())
    return g, S, dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3))


def kind_of(p):
    return (p.K, p.stride, p.pad, bool(p.transposed))


def packed_weights(p, o):
    """the flat weight buffer the kernel of a fwd / tr / dgrad case reads: fwd: the case's own buffer; tr: models/conv_f32._packed; dgrad:
    models/conv_f32.dgrad_layout -- the binding's packing is under test"""
    from octa_autosegmentation_amd.models import conv_f32
    if p.kind == "fwd":
        return o["wbuf"]
    if p.kind == "tr":
        return conv_f32._packed(o["w"], True).reshape(-1)
    return conv_f32.dgrad_layout(o["w"], kind_of(p)).reshape(-1)


def reference(p, o, cus=NUM_CUS[0]):
    if p.kind == "wgrad":
        a, b = (o["dy"], o["x"]) if p.transposed else (o["x"], o["dy"])
        r = SimpleNamespace()
        r.g, r.Sg, r.db, r.Sdb = wgrad_reference(a, b, p.K, p.stride, p.pad)
        return r
    src = o["dy"] if p.kind == "dgrad" else o["x"]
    return assemble(src, packed_weights(p, o), launches(p, cus), o.get("bias"))


def ratio(got, ref, tol):
    """the largest error / bound over EVERY element; an error where the bound is 0, or a NaN, counts as inf"""
    got = got.double().reshape(ref.shape)
    err = (got - ref).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / tol)
    q = torch.where(torch.isnan(got), torch.full_like(q, float("inf")), q)
    return q.max().item() if q.numel() else 0.0


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
# name: (the instantiations the case is listed under for 256 compute units, in launch order, params)

def _in_size(out, K, S, pad, extra=0):
    return (out - 1) * S + K - 2 * pad + extra


def _fwd_cases():
    c = {}

    def add(name, insts, K, S, out, extra=0, **kw):
        assert name not in c
        pad = kw.pop("pad", 1 if K == 4 else K // 2)
        c[name] = (insts, params("fwd", K=K, stride=S, pad=pad, H=_in_size(out[0], K, S, pad, extra), W=_in_size(out[1], K, S, pad, extra), **kw))

    for K, S in ((1, 1), (3, 1), (3, 2), (4, 1), (7, 1)):
        k, t = kc(K, S), f"k{K}s{S}_"
        n, w = [inst(K, S, 1)], [inst(K, S, 2)]
        s2 = w if S == 2 else n                      # stride 2 is wide whenever Cout > 32; stride 1 needs more than 128 tiles (256 CUs)
        add(t + "wo31_ho7", n, K, S, (7, 31), Cin=max(k - 1, 1), Cout=31)
        add(t + "wo32_ho8", n, K, S, (8, 32), Cin=k, Cout=32, extra=S - 1)
        add(t + "wo33_ho9_n3", s2, K, S, (9, 33), N=3, Cin=k + 1, Cout=33)
        add(t + "c1", n, K, S, (3, 5), Cin=1, Cout=1)
        add(t + "cout40", s2, K, S, (9, 33), Cin=2, Cout=40, extra=S - 1)
        add(t + "cout64_nobias", s2, K, S, (7, 32), Cin=2, Cout=64, bias=0)
        add(t + "cout72_n3", s2, K, S, (8, 33), N=3, Cin=k + 1, Cout=72)
    # 160 tiles of 8 x 32: the 64-channel workgroup at stride 1, on 256 and on 304 compute units
    add("k1s1_wide", [inst(1, 1, 2)], 1, 1, (40, 512), N=2, Cin=8, Cout=40, real=False)
    add("k3s1_wide", [inst(3, 1, 2)], 3, 1, (40, 512), N=2, Cin=4, Cout=64, real=False)
    add("k4s1_wide", [inst(4, 1, 2)], 4, 1, (40, 512), N=2, Cin=3, Cout=40, real=False)
    add("k7s1_wide", [inst(7, 1, 2)], 7, 1, (40, 512), N=2, Cin=2, Cout=64, real=False)
    # every padding supported() accepts: 0 .. K / 2 (the defaults above are 1, 1, 3)
    add("k3s1_pad0", [inst(3, 1, 1)], 3, 1, (7, 33), pad=0, Cin=9, Cout=5)
    add("k3s2_pad0", [inst(3, 2, 1)], 3, 2, (7, 33), pad=0, Cin=5, Cout=5)
    add("k4s1_pad0", [inst(4, 1, 1)], 4, 1, (9, 31), pad=0, Cin=5, Cout=7)
    add("k4s1_pad2", [inst(4, 1, 1)], 4, 1, (9, 33), pad=2, Cin=3, Cout=7, N=2)
    for pad in (0, 1, 2):
        add(f"k7s1_pad{pad}", [inst(7, 1, 1)], 7, 1, (7 + pad, 33), pad=pad, Cin=3, Cout=3)
    # a view of a larger packed tensor: rows cout_w apart, a nonzero offset
    add("k3s1_coutw", [inst(3, 1, 1)], 3, 1, (9, 33), N=2, Cin=9, Cout=33, cout_w=50, w_off=7)
    # one of the four 1x1 products of a 2x2 transposed convolution, stored scattered: Wp [Cin][4][Cout], tap 2a + b
    for a in (0, 1):
        for b in (0, 1):
            add(f"k1s1_scatter_{a}{b}", [inst(1, 1, 1)], 1, 1, (9, 33), N=2, Cin=5, Cout=20, cout_w=80, w_off=(2 * a + b) * 20, scatter=(2, a, b), bias=int(a != b))
    add("k3s2_scatter_10", [inst(3, 2, 2)], 3, 2, (3, 33), Cin=3, Cout=40, scatter=(2, 1, 0))
    return c


def _tr_cases():
    t = [inst(1, 1, 2, True)]
    return {"24_20_n2": (t, params("tr", N=2, Cin=24, Cout=20, H=9, W=33)), "1_1": (t, params("tr", Cin=1, Cout=1, H=1, W=1)),
            "9_33": (t, params("tr", Cin=9, Cout=33, H=8, W=32)), "7_64_n3": (t, params("tr", N=3, Cin=7, Cout=64, H=7, W=31)),
            "8_72": (t, params("tr", Cin=8, Cout=72, H=3, W=5))}


def _dgrad_cases():
    c = {}

    def add(name, insts, kind, **kw):
        assert name not in c
        K, S, pad, tr = kind
        c[name] = (insts, params("dgrad", K=K, stride=S, pad=pad, transposed=int(tr), **kw))

    n1, n3 = [inst(1, 1, 1)], [inst(3, 1, 1)]
    add("c11_24_20", n1, (1, 1, 0, False), N=2, Cin=24, Cout=20, H=9, W=33)
    add("c31_wo31", n3, (3, 1, 1, False), Cin=31, Cout=7, H=7, W=31)
    add("c31_wo32", n3, (3, 1, 1, False), Cin=32, Cout=8, H=8, W=32)
    add("c31_wo33_n3", n3, (3, 1, 1, False), N=3, Cin=33, Cout=9, H=9, W=33)
    add("c31_1_1", n3, (3, 1, 1, False), Cin=1, Cout=1, H=3, W=5)
    add("c31_40_2", n3, (3, 1, 1, False), Cin=40, Cout=2, H=5, W=33)
    add("c31_72_3", n3, (3, 1, 1, False), N=2, Cin=72, Cout=3, H=9, W=7)
    # 3x3 stride 2: the parity classes (0,0) 1x1, (0,1), (1,0), (1,1) 2x2; a map one pixel high / wide has no odd rows / columns
    s2 = [inst(1, 1, 1)] + [inst(2, 1, 1)] * 3
    add("c32_1x5", s2[:2], (3, 2, 1, False), Cin=5, Cout=7, H=1, W=5)
    add("c32_5x1", s2[:2], (3, 2, 1, False), Cin=7, Cout=5, H=5, W=1)
    add("c32_1x1", s2[:1], (3, 2, 1, False), Cin=3, Cout=3, H=1, W=1)
    add("c32_odd_n3", s2, (3, 2, 1, False), N=3, Cin=33, Cout=5, H=9, W=65)
    add("c32_even", s2, (3, 2, 1, False), N=2, Cin=31, Cout=9, H=16, W=66)
    add("c32_odd_even", s2, (3, 2, 1, False), Cin=1, Cout=1, H=7, W=64)
    # classes of 40 x 512 pixels in two images: 160 tiles, the 64-channel workgroup of <2,1> (and of <1,1> for class (0,0)); dx is 26 MB
    add("c32_wide", [inst(1, 1, 2)] + [inst(2, 1, 2)] * 3, (3, 2, 1, False), N=2, Cin=40, Cout=4, H=80, W=1024, real=False)
    add("t11_24_20", n1, (1, 1, 0, True), N=2, Cin=24, Cout=20, H=9, W=33)
    add("t22_24_20", [inst(2, 2, 1)], (2, 2, 0, True), N=2, Cin=24, Cout=20, H=5, W=17)
    add("t22_1_1", [inst(2, 2, 1)], (2, 2, 0, True), Cin=1, Cout=1, H=1, W=1)
    add("t22_40_5_n3", [inst(2, 2, 2)], (2, 2, 0, True), N=3, Cin=40, Cout=5, H=9, W=33)
    add("t22_72_3", [inst(2, 2, 2)], (2, 2, 0, True), Cin=72, Cout=3, H=8, W=32)
    return c


def _wgrad_cases():
    c = {}

    def add(name, kind, **kw):
        assert name not in c
        K, S, pad, tr = kind
        c[name] = ([f"wgrad<{K},{S}>"], params("wgrad", K=K, stride=S, pad=pad, transposed=int(tr), **kw))

    c11, c31, c32, t11, t22 = (1, 1, 0, False), (3, 1, 1, False), (3, 2, 1, False), (1, 1, 0, True), (2, 2, 0, True)
    add("c31_7x31_1_1", c31, Cin=1, Cout=1, H=7, W=31)
    add("c31_8x32", c31, Cin=32, Cout=31, H=8, W=32)
    add("c31_9x33_n3", c31, N=3, Cin=33, Cout=33, H=9, W=33)             # bias: 891 pixels, chunks of 14 cross the image boundaries (297)
    add("c11_7x31", c11, Cin=33, Cout=1, H=7, W=31)
    add("c11_9x33_n3", c11, N=3, Cin=9, Cout=33, H=9, W=33)
    add("c11_bias_35", c11, Cin=3, Cout=5, H=5, W=7)                       # bias: fewer pixels than DB_CHUNKS
    # stride 2: tiles of TH = 2 rows
    add("c32_ho1", c32, Cin=33, Cout=33, H=1, W=61)
    add("c32_ho2_n3", c32, N=3, Cin=5, Cout=40, H=4, W=64)
    add("c32_ho3", c32, Cin=32, Cout=1, H=5, W=65)
    add("t22_ho1", t22, Cin=24, Cout=20, H=1, W=31)
    add("t22_ho2_n3", t22, N=3, Cin=33, Cout=33, H=2, W=32)
    add("t22_ho3", t22, Cin=1, Cout=1, H=3, W=33)
    add("t11_24_20", t11, N=2, Cin=24, Cout=20, H=9, W=33)
    # two rounds, the second ragged: 64 channel blocks -> 16 chunks, 18 tiles in three images: chunks 0 and 1 take tiles (0, 16), (1, 17) of
    # images 0 and 2; 16 blocks -> 64 chunks, 66 tiles (W = 1: one column of tiles)
    add("c11_rounds", c11, N=3, Cin=256, Cout=256, H=16, W=65, real=False)
    add("c31_rounds", c31, N=3, Cin=128, Cout=128, H=176, W=1, real=False)
    add("c32_rounds", c32, N=3, Cin=128, Cout=128, H=87, W=1, real=False)
    add("t22_rounds", t22, N=3, Cin=128, Cout=128, H=44, W=1, real=False)
    return c


FAMILIES = {"fwd": _fwd_cases(), "tr": _tr_cases(), "dgrad": _dgrad_cases(), "wgrad": _wgrad_cases()}
ALL = [(fam, name, var) for fam, cases in FAMILIES.items() for name, (_, p) in cases.items() for var in ("exact", "real") if var == "exact" or p.real]


def _seed(fam, name, var):
    return 5000 + 1000 * KINDS.index(fam) + 3 * sorted(FAMILIES[fam]).index(name) + (var == "real")


def _quarters(shape, lim, gen, zero_half=False, unit=4):
    """multiples of 1 / unit in [-lim, lim]"""
    v = torch.randint(-unit * lim, unit * lim + 1, shape, generator=gen).float() / unit
    if zero_half:
        v = v * (torch.rand(shape, generator=gen) < 0.5)
    return v


def weight_shape(p):
    return (p.Cin, p.Cout, p.K, p.K) if p.transposed else (p.Cout, p.Cin, p.K, p.K)


@functools.lru_cache(maxsize=None)
def case(fam, name, var, num_cus=NUM_CUS[0]):
    """-> SimpleNamespace(p, insts, Ls = the launches (fwd / tr / dgrad) or d = the plan (wgrad), ops = the operands on the CPU). Drawn on the
    CPU from a generator seeded per case, so that the CPU proof and the GPU test see the same numbers. Asserts that the mirror of the dispatch
    names the instantiations the case is listed under (256 compute units; the wide and the stride-2 cases hold for 304 too)."""
    insts, p = FAMILIES[fam][name]
    gen = torch.Generator().manual_seed(_seed(fam, name, var))
    exact = var == "exact"
    c = SimpleNamespace(fam=fam, name=name, var=var, p=p, insts=insts)
    act = (lambda *sh: _quarters(sh, 3, gen)) if exact else (lambda *sh: torch.randn(sh, generator=gen))
    wgt = (lambda *sh: _quarters(sh, 2, gen, zero_half=True)) if exact else (lambda *sh: torch.randn(sh, generator=gen) / (p.K * p.K * 4) ** 0.5)
    o = {}
    if fam == "fwd":
        o["x"] = act(p.N, p.Cin, p.H, p.W)
        o["wbuf"] = wgt(p.w_off + p.Cin * p.K * p.K * p.cout_w)           # the gaps of a view hold weights too: reading them is wrong
        if p.bias:
            o["bias"] = _quarters((p.Cout,), 2, gen, unit=16) if exact else torch.randn((p.Cout,), generator=gen)
    elif fam == "tr":
        o["x"], o["w"] = act(p.N, p.Cin, p.H, p.W), wgt(*weight_shape(p))
    elif fam == "dgrad":
        o["dy"], o["w"] = act(p.N, p.Cout, p.Ho, p.Wo), wgt(*weight_shape(p))
    else:
        o["x"], o["dy"] = act(p.N, p.Cin, p.H, p.W), act(p.N, p.Cout, p.Ho, p.Wo)
    c.ops = o
    if fam == "wgrad":
        c.d = wgrad_dispatch(p)
        assert c.d is not None and [c.d.inst] == insts, f"{fam}/{name} would run {c.d and c.d.inst}, listed under {insts}"
    else:
        c.Ls = launches(p, num_cus)
        got = c.Ls and [L.inst for L in c.Ls]
        assert got == insts, f"{fam}/{name} would run {got} on {num_cus} compute units, not the kernels it is listed under ({insts})"
    return c


def ref_of(c, ops=None, num_cus=NUM_CUS[0]):
    """reference(...) of a case on its operands (ops: the same operands on another device); an exact case asserts its premise"""
    r = reference(c.p, c.ops if ops is None else ops, num_cus)
    if c.var == "exact":
        smax = max(r.Sg.max().item(), r.Sdb.max().item()) if c.fam == "wgrad" else r.S.max().item()
        assert smax < 2.0 ** 20, f"{c.fam}/{c.name}: sums reach {smax}, not exact in fp32"
    return r


@functools.lru_cache(maxsize=None)
def ref_cpu(fam, name, var):
    return ref_of(case(fam, name, var))


def _bits(t):
    return t.contiguous().view(torch.int32)


def expected_bits(r):
    """exact case, fwd / tr / dgrad: the bits of the whole output image: the reference where a launch writes, the sentinel elsewhere"""
    want = _bits(r.ref.float()).clone()
    want[:, :, ~r.written] = SENT_BITS
    return want


def check(c, r, got, worst=None):
    """got: fwd / tr / dgrad: y = the output image as the kernels left it (fp32, sentinel-filled before the call); wgrad: dw, db.
    Exact case: bit equality with the one legal result; real-valued case: EVERY element inside its bound, every unwritten element still the
    sentinel. -> name -> error / bound (0 or inf for an exact case); worst, if given, keeps the largest ratio per (family, output)."""
    rat = {}
    if c.fam == "wgrad":
        for k, ref, S, D in (("dw", r.g, r.Sg, c.d.D), ("db", r.db, r.Sdb, c.d.D_bias)):
            g = got[k]
            if g is None:
                continue
            if g.dtype != torch.float32 or g.shape != ref.shape:
                rat[k] = float("inf")
            elif c.var == "exact":
                rat[k] = 0.0 if torch.equal(g, ref.float()) and torch.equal(ref.float().double(), ref) else float("inf")
            else:
                rat[k] = ratio(g, ref, D * U24 * S)
    else:
        y = got["y"]
        if y.dtype != torch.float32 or y.shape != r.ref.shape:
            rat["y"] = float("inf")
        elif c.var == "exact":
            rat["y"] = 0.0 if torch.equal(_bits(y), expected_bits(r)) and torch.equal(r.ref.float().double(), r.ref) else float("inf")
        else:
            rat["y"] = ratio(y[:, :, r.written], r.ref[:, :, r.written], (r.D * U24 * r.S)[:, :, r.written])
            rat["untouched"] = 0.0 if bool((_bits(y)[:, :, ~r.written] == SENT_BITS).all()) else float("inf")
    if worst is not None and c.var == "real":
        for k, v in rat.items():
            worst[f"{c.fam}.{k}"] = max(worst.get(f"{c.fam}.{k}", 0.0), v)
    return rat


# ---- calls the host code has to refuse (tests/test_conv_f32_exact_gpu.py makes them with full-size buffers; tests/test_conv_f32_ref.py asserts
# that the mirror refuses each) -----------------------------------------------------------------------------------------------------------------
REFUSALS = {
    "fwd_scatter_3": params("fwd", scatter=(3, 0, 0)),
    "fwd_scatter_off_y": params("fwd", scatter=(2, 2, 0)),
    "fwd_scatter_off_x": params("fwd", scatter=(1, 0, 1)),
    "fwd_scatter_negative": params("fwd", scatter=(2, 0, -1)),
    "fwd_ho_beyond": params("fwd", Ho=9),
    "fwd_wo_beyond_s2": params("fwd", stride=2, H=9, W=9, Wo=6),
    "fwd_pad0_beyond": params("fwd", pad=0, Ho=7, Wo=6),
    "fwd_k5": params("fwd", K=5, pad=2),
    "fwd_k3_s3": params("fwd", K=3, stride=3, H=9, W=9),
    "fwd_k7_s2": params("fwd", K=7, stride=2, H=9, W=9),
    "fwd_cout_w_short": params("fwd", cout_w=31),
    "dgrad_k3_pad0": params("dgrad", K=3, pad=0),
    "dgrad_k4": params("dgrad", K=4, pad=1),
    "dgrad_k7": params("dgrad", K=7, pad=3),
    "dgrad_k3_s2_pad0": params("dgrad", K=3, stride=2, pad=0),
    "dgrad_t3": params("dgrad", K=3, stride=3, pad=0, transposed=1),
    "dgrad_t2_s1": params("dgrad", K=2, stride=1, pad=0, transposed=1, Ho=9, Wo=9),
    "dgrad_dy_high": params("dgrad", Ho=9),
    "dgrad_dy_narrow_s2": params("dgrad", stride=2, H=9, W=9, Wo=4),
    "dgrad_t2_dy_small": params("dgrad", K=2, stride=2, transposed=1, Ho=8, Wo=16),
    "wgrad_pad_3": params("wgrad", pad=3),
    "wgrad_k1_pad_1": params("wgrad", K=1, pad=1, Ho=8, Wo=8),
    "wgrad_ho_beyond": params("wgrad", Ho=9),
    "wgrad_k4": params("wgrad", K=4, pad=1),
    "wgrad_k2_s1": params("wgrad", K=2, pad=0),
    "wgrad_ws_short": params("wgrad", ws_short=1),
    "wgrad_ws_short_s2": params("wgrad", stride=2, ws_short=1),
    "tr_misaligned": params("tr", misalign=1),
}
