"""Proves tests/_head_ref.py without a GPU. An emulation of the arithmetic of csrc/head.hip in torch on the CPU -- weights rounded to bf16, the
32 products of one MFMA instruction added to the accumulator in order, the forward starting from the bias, a wave's dw / db accumulator
running over the tiles of its workgroup, the four waves folded in wave order, headn_reduce_kernel's 16 streams, one round-to-nearest-even to
bf16 on store, and the store through the four-pixel groups of head_group / head_step into a buffer of NaNs -- gives the one legal result on
every exact case, in forward and in reversed summation order, and stays inside every bound on every real-valued case; the same arithmetic in
float64 with every rounding replaced by a signed error at the edge of what the model grants stays inside too; each of a list of wrong
kernels (mutants of the emulation) breaks an equality or a bound on a case the test names; and the mirror of the host rules shows which
instantiations and loop trips the case list reaches. The loop cases run here at a reduced size (the sizes _head_ref's formulas give for 2
compute units): the arithmetic is the same, the tensors are not 20 MB. This is the evidence that the GPU tests can pass for a right kernel
and fail for a wrong one."""
import functools

import pytest
import torch

import _head_ref as hr

U = hr.U24
SMALL_CUS = 2            # the loop cases' stand-in for the CU count on the CPU
NAN = float("nan")


def _cus_of(name):
    return SMALL_CUS if name in hr.LOOP else hr.NUM_CUS[0]


def _trunc_bf16(v):
    return (v.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def _arith(push, seed=0):
    """-> (dtype, add(a, b), rnd(v) = the bf16 store). push None: fp32 as the kernel; (s_r, s_b, th): float64, every fp32 addition off by
    th * u of its result with sign s_r (0: a random sign per element and addition), the bf16 store off by th * 2^-8 with sign s_b"""
    if push is None:
        return torch.float32, (lambda a, b: a + b), (lambda v: v.bfloat16().float())
    s_r, s_b, th = push
    gen = torch.Generator().manual_seed(seed)

    def add(a, b):
        r = a + b
        s = s_r if s_r else torch.randint(0, 2, r.shape, generator=gen).double() * 2.0 - 1.0
        return r * (1.0 + th * U * s)

    return torch.float64, add, (lambda v: v * (1.0 + th * hr.HALF_BF16 * s_b))


def _store_map(N, hw, mut):
    """flat pixel -> (image, pixel in image, stored?) as the four-pixel groups of a tile place it (tiles start at multiples of 4)"""
    npix = N * hw
    p = torch.arange(npix)
    gs = p - p % 4
    q = gs % hw + (p - gs)
    gn = gs // hw
    if mut == "step_if":                     # `if` for the `while` of head_step
        over = (q >= hw).long()
        n, q = gn + over, q - hw * over
    elif mut == "seam_prev":                 # the pixel behind a seam goes to the previous image's row
        n, q = gn, q % hw
    else:
        n, q = gn + q // hw, q % hw
    keep = gs + 4 <= npix if mut == "drop_tail" else torch.ones(npix, dtype=torch.bool)
    return n, q, keep


def emulate(c, mut=None, rev=False, push=None, stale=None):
    """-> y [N][Cout][hw], dx [N][hw][Cin] (bf16 values in the working type; NaN where nothing was stored), dw [Cout][Cin], db [Cout]"""
    p, d, o, N, hw = c.p, c.d, c.ops, c.N, c.hw
    dt, add, rnd = _arith(push, seed=len(c.name))
    if mut == "trunc_out":
        rnd = _trunc_bf16
    Cin, Cout, npix = p.Cin, p.Cout, N * hw
    order = (lambda n: range(n - 1, -1, -1)) if rev else range
    w32 = o["w"].float()
    wq = (_trunc_bf16(w32) if mut == "trunc_w" else w32.bfloat16().float()).to(dt)
    x = o["x"].to(dt).reshape(npix, Cin)
    dy = o["dy"].to(dt).permute(0, 2, 1).reshape(npix, Cout)
    bias = o["b"].to(dt) if o["b"] is not None else torch.zeros(Cout, dtype=dt)

    # forward: the accumulator starts as the bias; KS instructions of 32 products
    acc = (torch.zeros(Cout, dtype=dt) if mut == "bias_after" else bias).expand(npix, Cout).clone()
    for ks in order(Cin // 32):
        for j in order(32):
            ch = ks * 32 + j
            acc = add(acc, x[:, ch:ch + 1] * wq[None, :, ch])
    yv = rnd(acc)
    if mut == "bias_after":
        yv = rnd(add(yv.to(dt), bias[None, :]))
    n_i, q_i, keep = _store_map(N, hw, mut)
    if mut == "trip2":                       # the grid-stride loops make one trip only
        keep = keep & (torch.arange(npix) < d.fwd_wgs * hr.TP)
    addr = (n_i[:, None] * Cout + torch.arange(Cout)[None, :]) * hw + q_i[:, None]
    ok = keep[:, None] & (addr < N * Cout * hw)
    y = torch.full((N * Cout * hw,), NAN, dtype=yv.dtype)
    y[addr[ok]] = yv[ok]
    y = y.view(N, Cout, hw)

    # dx: KT instructions over the padded output channels (zero weights there; the staged dy rows there are zero too)
    wd = o["w"].to(dt) if mut == "dx_unrounded" else wq
    if mut == "dx_wT":
        wd = wd.reshape(Cin, Cout).t().contiguous()
    wpad = torch.zeros(d.KP, Cin, dtype=dt)
    wpad[:Cout] = wd
    dyp = torch.zeros(npix, d.KP, dtype=dt)
    if mut == "pad_rows":                    # LDS rows >= Cout left as they were: any bit pattern, a non-finite one among them
        dyp.fill_(float("inf"))
    dyp[:, :Cout] = dy
    acc = torch.zeros(npix, Cin, dtype=dt)
    for ks in order(d.KT):
        for j in order(32):
            oo = ks * 32 + j
            acc = add(acc, dyp[:, oo:oo + 1] * wpad[oo][None, :])
    dx = rnd(acc)
    if mut == "trip2":
        dx[d.bwd_wgs * hr.TP:] = NAN
    dx = dx.view(N, hw, Cin)

    # dw, db: workgroup b takes tiles b, b + nparts, ...; wave v the pixels 64 v .. 64 v + 63 of a tile, two instructions of 32
    nparts, trips = d.nparts, d.bwd_trips
    tot = trips * nparts * hr.TP
    dz, xz = torch.zeros(tot, Cout, dtype=dt), torch.zeros(tot, Cin, dtype=dt)
    dz[:npix], xz[:npix] = dy, x
    dz, xz = dz.view(trips, nparts, 4, 64, Cout), xz.view(trips, nparts, 4, 64, Cin)
    aw, ab = torch.zeros(nparts, 4, Cout, Cin, dtype=dt), torch.zeros(nparts, 4, Cout, dtype=dt)
    for t in order(1 if mut == "trip2" else trips):
        for j in order(64):
            dd, xx = dz[t, :, :, j], xz[t, :, :, j]
            aw = add(aw, dd[..., :, None] * xx[..., None, :])
            ab = add(ab, dd)
    pw, pb = aw[:, 0], ab[:, 0]
    for v in range(1, 4):
        pw, pb = add(pw, aw[:, v]), add(pb, ab[:, v])
    if mut == "db_bf16":
        pb = pb.bfloat16().to(dt)
    parts = torch.cat((pw.reshape(nparts, -1), pb), 1)
    if mut == "stale":                       # the workspace still holds a partial of an earlier, larger call and the reduction reads it
        parts = torch.cat((parts, stale.to(dt).reshape(1, -1)), 0)
    if mut == "reduce16":
        parts = parts[:hr.RED_SPLIT]
    streams = []
    for sp in range(hr.RED_SPLIT):
        a = torch.zeros(parts.shape[1], dtype=dt)
        for b in (reversed(range(sp, parts.shape[0], hr.RED_SPLIT)) if rev else range(sp, parts.shape[0], hr.RED_SPLIT)):
            a = add(a, parts[b])
        streams.append(a)
    if rev:
        streams.reverse()
    tsum = streams[0]
    for s in streams[1:]:
        tsum = add(tsum, s)
    got = dict(y=y, dx=dx, dw=tsum[:Cout * Cin].view(Cout, Cin))
    if p.db:
        got["db"] = tsum[Cout * Cin:]
    return got


@functools.lru_cache(maxsize=None)
def _prepared(name, var):
    c = hr.case(name, var, _cus_of(name))
    return c, hr.ref_cpu(name, var, _cus_of(name))


def _fmt(rat):
    return {k: float(f"{v:.4g}") for k, v in rat.items()}


# ---- the case list and the mirror of the host rules ---------------------------------------------------------------------------------------

def test_case_list_reaches_every_instantiation_and_every_loop():
    for cus in hr.NUM_CUS:
        fwd, bwd = set(), set()
        for name in hr.CASES:
            p = hr.CASES[name]
            N, hw = hr.shape_of(name, cus)
            d = hr.dispatch(N, hw, p.Cin, p.Cout, cus)
            fwd.add(d.fwd)
            bwd.add(d.bwd)
            if p.loop:
                assert N > 1 and hw % 2 == 1
                assert (d.fwd_trips if p.loop == "fwd" else d.bwd_trips) >= 2, (name, cus, vars(d))
                assert N * hw * p.Cin * 2 <= 48 * 2 ** 20          # the largest input
            else:
                assert d.fwd_trips == d.bwd_trips == 1
        print(cus, "CUs: forward", len(fwd), "of", len(hr.fwd_instantiations()), "backward", len(bwd), "of", len(hr.bwd_instantiations()))
        assert fwd == hr.fwd_instantiations() and bwd == hr.bwd_instantiations()
        # the named loop sizes: one forward workgroup takes a second tile / every one takes two and three take a third; the backward likewise,
        # and the Cout 33 case runs KP = 64 with 31 padded rows of s_dy
        a, b = (hr.dispatch(*hr.shape_of(n, cus), 32, 2, cus) for n in ("loop_fwd_a", "loop_fwd_b"))
        assert a.ntiles == 4 * cus + 2 and a.fwd_trips == 2 and b.ntiles == 8 * cus + 4 and b.fwd_trips == 3
        a, b = hr.dispatch(*hr.shape_of("loop_bwd_a", cus), 32, 2, cus), hr.dispatch(*hr.shape_of("loop_bwd_b", cus), 32, 33, cus)
        assert a.ntiles == 2 * cus + 2 and a.bwd_trips == 2 and b.ntiles == 4 * cus + 2 and b.bwd_trips == 3 and b.KP == 64
        assert a.nparts == b.nparts == 2 * cus > hr.RED_SPLIT
    # the reduction's loop over partials: 1, 15 and 16 partials make one trip, 17 a second in one stream, 33 a third
    assert [hr.case(f"red_{t}", "exact").d.nparts for t in (1, 15, 16, 17, 33)] == [1, 15, 16, 17, 33]
    # groups that span images, seams inside a tile, every residue of the address modulo 8 bytes
    assert {hr.CASES[n].hw for n in hr.CASES if n.startswith("span")} == {1, 2, 3}
    assert {(hr.CASES[n].off * 2 + 2 * hr.CASES[n].hw * k) % 8 for n in hr.CASES if n.startswith("align_hw35") for k in range(10)} == {0, 2, 4, 6}
    assert {(hr.CASES[n].off * 2) % 8 for n in hr.CASES if n.startswith("align_hw64")} == {0, 2, 4, 6}


def test_mirror_refuses_what_the_host_code_refuses():
    for name, (N, hw, Cin, Cout) in hr.REFUSALS.items():
        assert hr.refusal(N, hw, Cin, Cout) and hr.dispatch(N, hw, Cin, Cout, 256) is None, name
    assert hr.refusal(1, 2 ** 30 - 1, 32, 2) is None and hr.refusal(2 ** 15, 2 ** 15, 32, 2) is not None
    for name in hr.CASES:
        for cus in hr.NUM_CUS:
            assert hr.refusal(*hr.shape_of(name, cus), hr.CASES[name].Cin, hr.CASES[name].Cout) is None


def test_chain_counts():
    d = hr.dispatch(1, 33 * 256, 32, 3, 256)
    assert hr.chain(32, d) == dict(y=32, dx=32, dw=64 + 3 + 3 + 15, db=64 + 3 + 3 + 15)
    d = hr.dispatch(1, 256 * (4 * 256 + 1) + 2, 64, 33, 256)
    assert hr.chain(64, d) == dict(y=64, dx=64, dw=3 * 64 + 3 + 32 + 15, db=3 * 64 + 3 + 32 + 15)


def test_reference_agrees_with_autograd():
    c = hr.case("inst_ci32_co17", "real")
    o, r = c.ops, hr.ref_cpu("inst_ci32_co17", "real")
    x, w, b = o["x"].double().requires_grad_(True), hr.rbf(o["w"].double()).requires_grad_(True), o["b"].double().requires_grad_(True)
    y = torch.nn.functional.conv1d(x.permute(0, 2, 1), w[:, :, None], b)
    y.backward(o["dy"].double())
    for k, v in (("y", y.detach()), ("dx", x.grad), ("dw", w.grad), ("db", b.grad)):
        assert (v - r[k][0]).abs().max().item() <= 1e-12 * max(1.0, r[k][0].abs().max().item()), k


# ---- the emulation: one result on the exact cases, inside the bounds on the real-valued ones ------------------------------------------------

@pytest.mark.parametrize("name", list(hr.CASES))
def test_emulated_kernels_meet_the_definition(name):
    for var in [v for n, v in hr.ALL if n == name]:
        c, r = _prepared(name, var)
        rat = hr.check(c, r, emulate(c))
        print("RATIO", name, var, _fmt(rat), "D", c.D)
        if var == "exact":
            assert all(v == 0.0 for v in rat.values()), (name, rat)
            back = hr.check(c, r, emulate(c, rev=True))
            assert all(v == 0.0 for v in back.values()), (name, "reversed order", back)
        else:
            assert all(v <= 1.0 for v in rat.values()), (name, rat)


def test_worst_emulation_ratio():
    worst = {}
    for name, var in hr.ALL:
        if var == "real":
            c, r = _prepared(name, var)
            for k, v in hr.check(c, r, emulate(c)).items():
                worst[k] = max(worst.get(k, (0.0, ""))[0], v), name
    print("WORST emulation / bound", {k: (float(f"{v:.4g}"), n) for k, (v, n) in worst.items()})
    assert set(worst) == set(hr.OUTPUTS) and all(v <= 1.0 for v, _ in worst.values())


@pytest.mark.parametrize("name", ["span_n5_hw3_co5", "edge_n3_hw171", "inst_ci64_co33", "inst_ci32_co64", "red_33"])
def test_bounds_hold_at_the_edge_of_the_model(name):
    """every fp32 addition off by 0.99 u of its result and the bf16 store by 0.99 * 2^-8, all one way, against each other, and with random
    signs (0.99: the store's error is relative to the erring sum, a second-order term of 2^-8 of the first bound)"""
    c, r = _prepared(name, "real")
    worst = {}
    for s_r, s_b in ((1.0, 1.0), (-1.0, -1.0), (1.0, -1.0), (-1.0, 1.0), (0, 1.0)):
        rat = hr.check(c, r, emulate(c, push=(s_r, s_b, 0.99)))
        assert all(v <= 1.0 for v in rat.values()), (name, s_r, s_b, rat)
        for k, v in rat.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("PUSHED", name, _fmt(worst))
    assert worst["y"] > 0.5 and worst["dx"] > 0.5            # the bf16 bound is nearly reached; the fp32 ones as far as the signs line up


# ---- the mutants ---------------------------------------------------------------------------------------------------------------------------
# mutant -> (case, variant, the outputs that must notice). pad_rows: the padded rows of s_dy meet zero weights in dx and rows of dw / db that
# the reduction never reads, so finite leftovers change nothing; what shows is a non-finite bit pattern, which uninitialised LDS may hold
# (0 * inf = NaN in dx): the emulation leaves inf there.
MUTANTS = {
    "trunc_out": ("inst_ci32_co17", "real", ("y", "dx")),
    "trunc_w": ("inst_ci32_co17", "real", ("y", "dx")),
    "dx_unrounded": ("inst_ci32_co17", "real", ("dx",)),
    "bias_after": ("inst_ci32_co17", "real", ("y",)),
    "step_if": ("span_n7_hw1_co2", "exact", ("y",)),
    "drop_tail": ("edge_257", "exact", ("y",)),
    "seam_prev": ("edge_n3_hw171", "exact", ("y",)),
    "pad_rows": ("inst_ci32_co33", "exact", ("dx",)),
    "reduce16": ("red_17", "exact", ("dw", "db")),
    "stale": ("span_n7_hw1_co2", "exact", ("dw", "db")),
    "dx_wT": ("inst_ci32_co17", "exact", ("dx",)),
    "db_bf16": ("red_33", "real", ("db",)),
}


@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_mutant_is_rejected(mut):
    name, var, outs = MUTANTS[mut]
    c, r = _prepared(name, var)
    stale = None
    if mut == "stale":          # slot nparts of the workspace as an earlier, larger call of the same channel counts left it: one tile's sums
        big, rb = _prepared("span_n5_hw3_co2", "exact")
        stale = torch.cat((rb["dw"][0].reshape(-1), rb["db"][0]))
        assert stale.abs().max() > 0 and big.p.Cout == c.p.Cout and big.N * big.hw > c.N * c.hw
    rat = hr.check(c, r, emulate(c, mut=mut, stale=stale))
    print(mut, "on", name, var, _fmt(rat))
    for k in outs:
        assert not rat[k] <= 1.0, f"{k} of case {name} does not notice the mutant {mut}: {rat}"
    good = hr.check(c, r, emulate(c))
    assert all(v <= 1.0 for v in good.values())


def test_exact_variants_notice_the_rounding_mutants_too():
    """a truncating output pack and a bias added after the rounding change bits of an exact case whose sums need more than 8 bits"""
    c, r = _prepared("inst_ci64_co64", "exact")
    assert hr.check(c, r, emulate(c, mut="trunc_out"))["y"] == float("inf")
    assert hr.check(c, r, emulate(c, mut="bias_after"))["y"] == float("inf")


def test_loop_cases_notice_a_dropped_second_trip():
    """the reduced loop cases: without the later trips of the grid-stride loops y and dx keep unwritten elements and dw / db lose terms"""
    for name in hr.LOOP:
        c, r = _prepared(name, "exact")
        assert (c.d.fwd_trips if c.p.loop == "fwd" else c.d.bwd_trips) >= 2
        rat = hr.check(c, r, emulate(c, mut="trip2"))
        print(name, rat)
        assert rat["y" if c.p.loop == "fwd" else "dx"] == float("inf"), (name, rat)
        if c.p.loop == "bwd":
            assert rat["dw"] == rat["db"] == float("inf"), (name, rat)
