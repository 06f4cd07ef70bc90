"""The definition of "correct" for the N-channel 1x1 head of csrc/head.hip (headn_fwd_kernel, headn_bwd_kernel, headn_reduce_kernel): a
float64 reference by the formulas in that file's header, the two families of inputs it is applied to, the bound a correct kernel has to
meet on the second family, a mirror of the host code's rules, and the case list shared by tests/test_head_ref.py (CPU: proves reference and
bounds on an emulation of the kernels' arithmetic) and tests/test_head_exact_gpu.py (the kernels themselves). Plain torch, any device, no
native code. The method is that of tests/_conv_ref.py, whose rbf / once / ratio are used here.

    forward   y[n][o][q]  = bias[o] + sum_c x[n][q][c] W[o][c]          x NHWC bf16, y CHANNEL-FIRST bf16
    backward  dx[n][q][c] = sum_o dy[n][o][q] W[o][c]                   dy channel-first bf16, dx NHWC bf16
              dw[o][c]    = sum_{n,q} dy[n][o][q] x[n][q][c]            float32
              db[o]       = sum_{n,q} dy[n][o][q]                       float32
W = rbf(w): the weights reach the kernels as fp32 and are rounded to the nearest bf16 number (ties to even) inside them, in the forward's
B fragments and in the A fragments of dx alike; the bias stays fp32. Every reference also returns S, the sum of the magnitudes of the terms
of each output (the bias included).

EXACT cases. Activations and gradients are multiples of 2^-2 in [-3, 3], weights multiples of 2^-2 in [-2, 2] (about half of them zero),
the bias a multiple of 2^-4 in [-2, 2]; the loop cases draw all three from {-1, -1/2, 0, 1/2, 1}. Products are multiples of g = 2^-4
(2^-2 in the loop cases), the terms of db multiples of 2^-2 (2^-1); ref_of() asserts S < 2^24 g for every output, so every partial sum in
ANY order -- through the MFMA chain, the LDS fold of the waves, the workspace and the 16-way reduction -- is an fp32 number. A correct
kernel has ONE legal result: once(ref) for y and dx, the reference itself for dw and db, compared with torch.equal.

REAL-VALUED cases (weights ~ N(0, 1 / Cin) in fp32: no bf16 numbers). Every element:
    y, dx: |got - ref| <= 2^-8 |ref| + D * 2^-24 * S                   dw, db: |got - ref| <= D * 2^-24 * S
D (chain()) counts dependent fp32 roundings behind one accumulator, read from the kernels. One v_mfma_f32_16x16x32_bf16 adds 32 products to an
accumulator element: R_MFMA = 32 roundings, one per product, as a chain of fused multiply-adds would give (the order inside an instruction
is not documented here; any order that rounds once per product stays inside).
  y   the accumulator starts as the bias (no rounding) and takes KS = Cin / 32 instructions:                    Cin / 32 * R_MFMA
  dx  the accumulator starts at zero and takes KT = padded Cout / 32 instructions (the padding adds zeros):     KT * R_MFMA
  dw, db  a wave's accumulator takes two instructions per tile (its 64 pixels) over the `trips` tiles of its workgroup, the four waves are
      added in wave order in LDS (3), headn_reduce_kernel adds the partials of a stream in order (ceil(nparts / 16), the first to zero) and
      the 16 streams in order (15):                                       2 * trips * R_MFMA + 3 + ceil(nparts / 16) + 15
      db is the same product with a B operand of ones.

THE HOST RULES, as read from headn_check, octa_headn_nhwc_fwd / _bwd and launch_fwd / launch_bwd: Cin 32 or 64, 2 <= Cout <= 64, N, hw > 0,
N * hw < 2^30; forward instantiation <Cin, NT = ceil(Cout / 16)> on min(ntiles, 4 * num_cus) workgroups, backward <Cin, KT = ceil(Cout / 32)>
on min(ntiles, 2 * num_cus) workgroups (= the number of partials), ntiles = ceil(N * hw / 256); a workgroup takes tiles b, b + workgroups, ...
"""
import functools
from types import SimpleNamespace

import torch

from _conv_ref import HALF_BF16, NUM_CUS, U24, once, ratio, rbf  # noqa: F401  (once / ratio: for the users of this module)

R_MFMA = 32                  # products, and roundings, per v_mfma_f32_16x16x32_bf16 and accumulator element (module docstring)
TP = 256                     # HEAD_TP: pixels per tile
RED_SPLIT = 16               # HEAD_RED_SPLIT
OUTPUTS = ("y", "dx", "dw", "db")


# ---- the host code's rules ---------------------------------------------------------------------------------------------------------------

def refusal(N, hw, Cin, Cout):
    """why headn_check refuses the shape, or None"""
    if N <= 0 or hw <= 0 or Cin not in (32, 64) or Cout < 2 or Cout > 64:
        return "unsupported shape"
    if hw > (2 ** 31 - 1) // 2 or N * hw > (2 ** 31 - 1) // 2:
        return "beyond the kernel's 2^30 limit"
    return None


def dispatch(N, hw, Cin, Cout, num_cus):
    """-> SimpleNamespace(fwd, bwd = the instantiations, ntiles, fwd_wgs, bwd_wgs = nparts, fwd_trips, bwd_trips, KT, KP), None if refused"""
    if refusal(N, hw, Cin, Cout):
        return None
    d = SimpleNamespace(NT=(Cout + 15) // 16, KT=(Cout + 31) // 32)
    d.KP = d.KT * 32
    d.fwd, d.bwd = f"fwd<{Cin},{d.NT}>", f"bwd<{Cin},{d.KT}>"
    d.ntiles = (N * hw + TP - 1) // TP
    d.fwd_wgs, d.bwd_wgs = min(d.ntiles, 4 * num_cus), min(d.ntiles, 2 * num_cus)
    d.fwd_trips, d.bwd_trips = -(-d.ntiles // d.fwd_wgs), -(-d.ntiles // d.bwd_wgs)
    d.nparts = d.bwd_wgs
    return d


def fwd_instantiations():
    return {f"fwd<{ci},{nt}>" for ci in (32, 64) for nt in (1, 2, 3, 4)}


def bwd_instantiations():
    return {f"bwd<{ci},{kt}>" for ci in (32, 64) for kt in (1, 2)}


def chain(Cin, d):
    """D per output: the longest chain of dependent fp32 roundings behind one element (module docstring)"""
    dwb = 2 * d.bwd_trips * R_MFMA + 3 + -(-d.nparts // RED_SPLIT) + (RED_SPLIT - 1)
    return dict(y=Cin // 32 * R_MFMA, dx=d.KT * R_MFMA, dw=dwb, db=dwb)


# ---- the float64 reference ---------------------------------------------------------------------------------------------------------------

def reference(o):
    """o: x [N][hw][Cin] bf16, w [Cout][Cin] fp32, b [Cout] fp32 or None, dy [N][Cout][hw] bf16 -> name -> (ref, S), float64"""
    x, dy, W = o["x"].double(), o["dy"].double(), rbf(o["w"].double())
    xa, dya, Wa = x.abs(), dy.abs(), W.abs()
    y, Sy = torch.einsum("nqc,oc->noq", x, W), torch.einsum("nqc,oc->noq", xa, Wa)
    if o.get("b") is not None:
        y, Sy = y + o["b"].double()[None, :, None], Sy + o["b"].double().abs()[None, :, None]
    return dict(y=(y, Sy), dx=(torch.einsum("noq,oc->nqc", dy, W), torch.einsum("noq,oc->nqc", dya, Wa)),
                dw=(torch.einsum("noq,nqc->oc", dy, x), torch.einsum("noq,nqc->oc", dya, xa)), db=(dy.sum((0, 2)), dya.sum((0, 2))))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
# name -> SimpleNamespace(N, hw (numbers, or functions of the CU count), Cin, Cout, off = element offset of y and dy from a 16-byte-aligned
# base, bias, db = False: a null pointer, real = the real-valued variant runs too, loop = None | 'fwd' | 'bwd': a workgroup of that kernel
# takes a second tile at 256 and at 304 compute units, tiles = the tile count the case is listed for)

def _odd_split(npix):
    """(N, hw) with N * hw = npix, N > 1 as small as possible and hw odd"""
    for n in range(2, 4097):
        if npix % n == 0 and (npix // n) % 2 == 1:
            return n, npix // n
    raise AssertionError(f"{npix} pixels do not split into N > 1 images of an odd size")


def _loop_pixels(kind, cus):
    """the loop sizes: 256 (4 c) + 256 + 5 and 256 (8 c + 3) + 1 pixels forward, 256 (2 c) + 256 + 5 and 256 (4 c + 1) + 2 backward, c compute
    units; a size without a split into N > 1 images of an odd hw moves up by 2 pixels (keeps the odd tail and the trips)"""
    npix = {"fwd_a": TP * (4 * cus) + TP + 5, "fwd_b": TP * (8 * cus + 3) + 1, "bwd_a": TP * (2 * cus) + TP + 5, "bwd_b": TP * (4 * cus + 1) + 2}[kind]
    while True:
        try:
            return _odd_split(npix)
        except AssertionError:
            npix += 2


def _cases():
    c = {}

    def add(name, N, hw, Cout, Cin=32, off=0, bias=True, db=True, real=True, loop=None, tiles=None):
        assert name not in c
        c[name] = SimpleNamespace(N=N, hw=hw, Cin=Cin, Cout=Cout, off=off, bias=bias, db=db, real=real, loop=loop, tiles=tiles)

    for n, hw in ((7, 1), (3, 2), (5, 3)):                  # a four-pixel group spans up to four images: the while of head_step
        for co in (2, 5):
            add(f"span_n{n}_hw{hw}_co{co}", n, hw, co)
    for hw in (35, 64):                                     # every alignment branch of the row moves (hw 64: always the 8-byte one at offset 0)
        for off in range(4):
            add(f"align_hw{hw}_off{off}", 2, hw, 5, off=off, real=off == 1)
    for hw in (255, 256, 257):
        add(f"edge_{hw}", 1, hw, 3)
    add("edge_n3_hw171", 3, 171, 3)                         # two seams, one inside a tile and one in the tile that also ends the tensor
    for ci in (32, 64):
        for co in (2, 16, 17, 32, 33, 48, 49, 64):
            add(f"inst_ci{ci}_co{co}", 2, 35, co, Cin=ci)
    for t in (1, 15, 16, 17, 33):                           # partials per stream of the reduction: 1, 1, 1, 2 (one stream), 3
        add(f"red_{t}", 1, TP * t - 5, 3, tiles=t)
    add("loop_fwd_a", lambda cus: _loop_pixels("fwd_a", cus)[0], lambda cus: _loop_pixels("fwd_a", cus)[1], 2, real=False, loop="fwd")
    add("loop_fwd_b", lambda cus: _loop_pixels("fwd_b", cus)[0], lambda cus: _loop_pixels("fwd_b", cus)[1], 2, real=False, loop="fwd")
    add("loop_bwd_a", lambda cus: _loop_pixels("bwd_a", cus)[0], lambda cus: _loop_pixels("bwd_a", cus)[1], 2, real=False, loop="bwd")
    add("loop_bwd_b", lambda cus: _loop_pixels("bwd_b", cus)[0], lambda cus: _loop_pixels("bwd_b", cus)[1], 33, real=False, loop="bwd")
    add("no_bias", 2, 35, 5, bias=False)
    add("no_db", 2, 35, 5, db=False)
    return c


CASES = _cases()
LOOP = [n for n, p in CASES.items() if p.loop]
SMALL = [n for n in CASES if n not in LOOP]
ALL = [(n, v) for n, p in CASES.items() for v in ("exact", "real") if v == "exact" or p.real]


def shape_of(name, num_cus):
    p = CASES[name]
    return (p.N(num_cus) if callable(p.N) else p.N), (p.hw(num_cus) if callable(p.hw) else p.hw)


def _grid(shape, lim, unit, gen, zero_half=False):
    """multiples of `unit` in [-lim, lim]"""
    k = round(lim / unit)
    v = torch.randint(-k, k + 1, shape, generator=gen).float() * unit
    if zero_half:
        v = v * (torch.rand(shape, generator=gen) < 0.5)
    return v


@functools.lru_cache(maxsize=None)
def case(name, var, num_cus=NUM_CUS[0]):
    """-> SimpleNamespace(name, var, p, N, hw, d = the dispatch, D = name -> chain, g = name -> granule (exact), ops = the operands on the CPU).
    Drawn on the CPU from a generator seeded per case, so that the CPU proof and the GPU test see the same numbers."""
    p = CASES[name]
    N, hw = shape_of(name, num_cus)
    c = SimpleNamespace(name=name, var=var, p=p, N=N, hw=hw, d=dispatch(N, hw, p.Cin, p.Cout, num_cus))
    assert c.d is not None, f"{name}: refused"
    if p.loop == "fwd":
        assert c.d.fwd_trips > 1 and N > 1 and hw % 2 == 1 and (N * hw) % 4, f"{name}: no forward workgroup takes a second tile at {num_cus} compute units"
    if p.loop == "bwd":
        assert c.d.bwd_trips > 1 and N > 1 and hw % 2 == 1 and (N * hw) % TP, f"{name}: no backward workgroup takes a second tile at {num_cus} compute units"
    if p.tiles is not None:
        assert c.d.ntiles == c.d.nparts == p.tiles, f"{name}: {c.d.ntiles} tiles, listed under {p.tiles}"
    c.D = chain(p.Cin, c.d)
    gen = torch.Generator().manual_seed(7000 + 2 * sorted(CASES).index(name) + (var == "real"))
    bf = torch.bfloat16
    if var == "exact":
        lim, wl, u = (1.0, 1.0, 0.5) if p.loop else (3.0, 2.0, 0.25)
        o = dict(x=_grid((N, hw, p.Cin), lim, u, gen).to(bf), dy=_grid((N, p.Cout, hw), lim, u, gen).to(bf),
                 w=_grid((p.Cout, p.Cin), wl, u, gen, zero_half=True), b=_grid((p.Cout,), wl, u * u, gen) if p.bias else None)
        c.g = dict(y=u * u, dx=u * u, dw=u * u, db=u)
    else:
        o = dict(x=torch.randn((N, hw, p.Cin), generator=gen).to(bf), dy=torch.randn((N, p.Cout, hw), generator=gen).to(bf),
                 w=torch.randn((p.Cout, p.Cin), generator=gen) / p.Cin ** 0.5, b=torch.randn((p.Cout,), generator=gen) if p.bias else None)
        assert not torch.equal(rbf(o["w"].double()), o["w"].double()), f"{name}: the weights are bf16 numbers"
    c.ops = o
    return c


def ref_of(c, ops=None):
    """reference(...) of a case on its operands (ops: the same operands on another device); an exact case asserts its premise"""
    r = reference(c.ops if ops is None else ops)
    if c.var == "exact":
        for k, (_, S) in r.items():
            assert S.max().item() < 2.0 ** 24 * c.g[k], f"{c.name}: the terms of {k} sum to {S.max().item()}, not exact in fp32"
    return r


@functools.lru_cache(maxsize=None)
def ref_cpu(name, var, num_cus=NUM_CUS[0]):
    return ref_of(case(name, var, num_cus))


def check(c, r, got):
    """got: name -> tensor as the kernel wrote it (y [N][Cout][hw], dx [N][hw][Cin] bf16 or their values in a wider type; dw [Cout][Cin],
    db [Cout] fp32; db absent where the case passes a null pointer). Exact case: bit equality with the one legal result; real-valued case:
    every element inside its bound. -> name -> error / bound (0 or inf for an exact case)"""
    rat = {}
    for k, v in got.items():
        ref, S = r[k]
        if v.shape != ref.shape:
            rat[k] = float("inf")
        elif c.var == "exact":
            want = once(ref) if k in ("y", "dx") else ref.float()
            same = torch.equal(v.to(want.dtype), want) and torch.equal(v.double(), want.double())
            rat[k] = 0.0 if same else float("inf")
        else:
            tol = c.D[k] * U24 * S + (HALF_BF16 * ref.abs() if k in ("y", "dx") else 0.0)
            rat[k] = ratio(v, ref, tol)
    return rat


# calls the host code has to refuse: name -> (N, hw, Cin, Cout) (tests/test_head_exact_gpu.py adds the null pointers)
REFUSALS = {"cin_48": (1, 16, 48, 4), "cin_16": (1, 16, 16, 4), "cin_128": (1, 16, 128, 4), "cout_1": (1, 16, 32, 1), "cout_65": (1, 16, 32, 65),
            "n_0": (0, 16, 32, 4), "hw_0": (1, 0, 32, 4), "pixels_2^30": (1024, 2 ** 20, 32, 4), "hw_2^30": (1, 2 ** 30, 64, 4)}
