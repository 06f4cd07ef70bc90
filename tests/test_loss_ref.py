"""Proves tests/_loss_ref.py without a GPU. An emulation of the arithmetic of csrc/loss.hip in torch on the CPU (fp32 elementwise, each
thread's K terms chained in fp32 in the kernel's own order and folded in double, the finish in double rounded to fp32, the gradient in
fp32 with one round-to-nearest-even to bf16) stays inside every bound on every case that tests/test_loss_gpu.py runs; the same
arithmetic with every error source pushed to the edge of what the model grants stays inside too; the hand-written float64 reference
agrees with torch.autograd of the plain composition; and each of a list of wrong kernels (mutants of the emulation) breaks a bound on a
case the test names. This is the evidence that the GPU tests can pass for a right kernel and fail for a wrong one."""
import functools

import pytest
import torch

import _loss_ref as lr

U = lr.U


def _bf16_trunc(v):
    return (v.float().view(torch.int32) & -65536).view(torch.float32)


def _chain(v, stride, K, skip=None):
    """sum over dim 1 of fp32 [rows][n] as the forward kernel forms it: thread j adds elements j, j + stride, ... in fp32 (K trips), the
    rest is double"""
    rows, n = v.shape
    v = torch.nn.functional.pad(v, (0, K * stride - n)).view(rows, K, stride)
    acc = torch.zeros(rows, stride, dtype=v.dtype)
    for k in range(K):
        if k != skip:
            acc = acc + v[:, k]
    return acc.double().sum(1)


def emulate(x, t, gout, cus=lr.CUS, nr=lr.NR, dr=lr.DR, bf16=False, mut=None):
    """-> sums [rows][4] float64, loss fp32, dx fp32 / bf16"""
    x, t = x.float(), t.float()
    rows, n = x.shape
    tt = (t > 0.5).float() if mut == "threshold" else t
    e = torch.exp(-x.abs())
    p = torch.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    terms = [p * tt, p, tt, x.clamp_min(0) - x * tt + torch.log1p(e)]
    stride = lr.grid_x(n, rows, cus, "fwd") * 256
    K = lr.trips(n, rows, cus, "fwd")
    if mut == "tail":
        terms = [torch.cat((m[:, :-1], torch.zeros(rows, 1)), 1) for m in terms]
    sums = torch.stack([_chain(m, stride, K, skip=1 if mut == "trip2" else None) for m in terms], 1)
    enr, edr = (0.0 if mut == "no_nr" else nr), (0.0 if mut == "no_dr" else dr)
    N, D = 2.0 * sums[:, 0] + enr, sums[:, 1] + sums[:, 2] + edr
    cnt = n if mut == "one_over_n" else rows * n
    loss = (((1.0 - N / D).mean() + sums[:, 3].sum() / cnt) / 2.0).float()
    # the backward takes the smoothing terms as fp32
    N, D = 2.0 * sums[:, 0] + (0.0 if mut == "no_nr" else lr.f32(nr)), sums[:, 1] + sums[:, 2] + (0.0 if mut == "no_dr" else lr.f32(dr))
    g = torch.tensor((1.0 if mut == "no_half" else 0.5) * (1.0 if mut == "no_gout" else gout), dtype=torch.float32)
    kd = (1.0 / ((1 if mut == "no_rows" else rows) * D * D)).float()[:, None]
    fN, fD, kb = N.float()[:, None], D.float()[:, None], torch.tensor(1.0 / cnt, dtype=torch.float32)
    ddice = -(2.0 * tt * fD - fN) * kd * p * (1.0 if mut == "p_not_pq" else (1.0 - p))
    dx = g * (ddice + (p - tt) * kb)
    if mut == "tail":
        dx[:, -1] = 0.0
    if mut == "trip2":
        sb = lr.grid_x(n, rows, cus, "bwd") * 256
        dx[:, sb:2 * sb] = 0.0
    if bf16:
        dx = _bf16_trunc(dx) if mut == "truncate" else dx.bfloat16()
    return dict(sums=sums, loss=loss, dx=dx)


def pushed(x, t, gout, signs, cus=lr.CUS, nr=lr.NR, dr=lr.DR, bf16=False, th=0.999):
    """The kernels' arithmetic in float64 with every error the model names put in by hand at th times its allowance (th keeps the
    second-order terms, 1e-5 of the first-order ones, out of the way): signs = (s_e, s_p, s_r, s_b) for exp, the sigmoid's own
    roundings, every other fp32 rounding, and the rounding to bf16, each +-1 or a tensor of +-1 per element."""
    s_e, s_p, s_r, s_b = signs
    x, t = x.double(), t.double()
    rows, n = x.shape
    rd = lambda v, s=None: v * (1.0 + th * U * (s_r if s is None else s))            # one fp32 rounding
    a = x.abs()
    e = torch.exp(-a) * (1.0 + th * s_e * (lr.C_E + lr.C_A * a) * U) + th * s_e * lr.FLOOR
    e = e.clamp_min(0.0)
    p = torch.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e)) * (1.0 + th * lr.C_P * U * s_p)
    l1p = torch.log1p(e) * (1.0 + th * lr.C_L * U * s_r)
    terms = [rd(p * t), p, t, rd(rd(x.clamp_min(0) - rd(x * t)) + l1p)]
    stride, K = lr.grid_x(n, rows, cus, "fwd") * 256, lr.trips(n, rows, cus, "fwd")
    sums = []
    for m in terms:
        m = torch.nn.functional.pad(m, (0, K * stride - n)).view(rows, K, stride)
        sr = s_r if not torch.is_tensor(s_r) else torch.nn.functional.pad(s_r, (0, K * stride - n), value=1.0).view(rows, K, stride)
        acc = m[:, 0]
        for k in range(1, K):
            acc = (acc + m[:, k]) * (1.0 + th * U * (sr if not torch.is_tensor(sr) else sr[:, k]))
        sums.append(acc.sum(1))
    sums = torch.stack(sums, 1)
    N, D = 2.0 * sums[:, 0] + nr, sums[:, 1] + sums[:, 2] + dr
    srs = s_r if not torch.is_tensor(s_r) else 1.0
    loss = ((1.0 - N / D).mean() + sums[:, 3].sum() / (rows * n)) / 2.0 * (1.0 + th * U * srs)
    N, D = 2.0 * sums[:, 0] + nr * (1.0 + th * U * srs), sums[:, 1] + sums[:, 2] + dr * (1.0 - th * U * srs)
    kd = rd(1.0 / (rows * D * D), srs)[:, None]
    # fD low and fN high (or the reverse) push 2 t fD - fN one way
    fN, fD = rd(N, -srs)[:, None], rd(D, srs)[:, None]
    ddice = rd(rd(-rd(rd(rd(2.0 * t * fD) - fN) * kd) * p) * rd(1.0 - p))
    dx = rd(gout / 2.0 * rd(ddice + rd(rd(p - t) * rd(1.0 / (rows * n), srs))))
    if bf16:
        dx = dx * (1.0 + th * 2.0 ** -8 * s_b)
    dx = dx + th * lr.FLOOR * s_b               # a flushed denormal
    return dict(sums=sums, loss=loss, dx=dx)


# ---- the cases, each with its reference and bounds computed once ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _prepared(cid, bf16=False):
    x, t, g = lr.case(cid, bf16=bf16)
    r = lr.reference(x, t, g)
    return x, t, g, r, lr.bounds(r, lr.trips(x.shape[1], x.shape[0], lr.CUS, "fwd"), bf16=bf16)


def test_cases_are_what_they_claim():
    for cid in lr.CASES:
        x, t, g, r, _ = _prepared(cid)
        assert (x[:, -1] == 3.0).logical_or(t.sum(1) == 0).all() and (t[:, -1] == 1.0).logical_or(t.sum(1) == 0).all()
        assert g == (1.0 if cid.startswith("1") else lr.f32(0.37))
    x, t, _, r, _ = _prepared("4-wide")
    assert (x.abs() >= 20).any() and ((x.abs() > 87.4) & (x.abs() < 103)).any() and (x.abs() > 104).any()
    for cid in ("6-empty-15", "6-empty-30"):
        _, t, _, r, _ = _prepared(cid)
        assert (t == 0).all() and (r.N == lr.NR).all()           # the numerator IS the smoothing term
    assert (_prepared("6-empty-30")[3].D < 2 * lr.DR).all()     # and so is most of the denominator
    assert (_prepared("5-empty-row")[1][0] == 0).all() and _prepared("3-soft")[1].frac().ne(0).any()
    assert (_prepared("7-full+15")[1] == 1).all()


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_emulated_kernels_are_within_every_bound(bf16):
    worst = {}
    for cid in lr.CASES:
        x, t, g, r, tol = _prepared(cid, bf16)
        rat = lr.ratios(r, tol, emulate(x, t, g, bf16=bf16))
        print(cid, {k: round(v, 4) for k, v in rat.items()})
        lr.assert_within(rat, cid)
        for k, v in rat.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("worst", {k: round(v, 4) for k, v in worst.items()})


def _sign_patterns(shape):
    gen = torch.Generator().manual_seed(99)
    rnd = lambda: torch.randint(0, 2, shape, generator=gen).double() * 2.0 - 1.0
    return [(1.0, 1.0, 1.0, 1.0), (-1.0, -1.0, -1.0, -1.0), (1.0, -1.0, -1.0, -1.0), (-1.0, 1.0, 1.0, 1.0), (1.0, 1.0, -1.0, 1.0),
            (-1.0, -1.0, 1.0, -1.0), (rnd(), rnd(), rnd(), rnd()), (rnd(), 1.0, rnd(), -1.0)]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_bounds_hold_at_the_edge_of_the_model(bf16):
    """signed worst cases: every error source at its allowance, all one way, exp against the rest, and at random per element"""
    worst = {}
    for cid in lr.CASES:
        x, t, g, r, tol = _prepared(cid, bf16)
        pats = _sign_patterns(tuple(x.shape))
        for i, signs in enumerate(pats if cid in lr.SMALL else pats[:3]):
            rat = lr.ratios(r, tol, pushed(x, t, g, signs, bf16=bf16))
            lr.assert_within(rat, f"{cid}, sign pattern {i}")
            for k, v in rat.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print("worst", {k: round(v, 4) for k, v in worst.items()})
    assert all(v > 0.3 for v in worst.values()), worst          # the pushed errors do come close: the bounds are not slack by much


@pytest.mark.parametrize("cid", lr.SMALL)
def test_reference_agrees_with_autograd_of_the_composition(cid):
    """loss and gradient of the hand-written reference against torch.autograd on (Dice(sigmoid) + BCEWithLogits) / 2 in float64"""
    x, t, g, r, _ = _prepared(cid)
    xd = x.double().requires_grad_(True)
    p = torch.sigmoid(xd)
    dice = torch.mean(1.0 - (2.0 * (p * t).sum(1) + lr.NR) / (p.sum(1) + t.double().sum(1) + lr.DR))
    loss = (dice + torch.nn.functional.binary_cross_entropy_with_logits(xd, t.double())) / 2.0
    (loss * g).backward()
    assert abs(loss.item() - r.loss.item()) <= 1e-13 * max(1.0, abs(r.loss.item()))
    # autograd forms 1 - p by subtraction: 2^-53 absolute in p, times the factor of p (1 - p)
    F = (2.0 * r.t * r.D[:, None] + r.N[:, None]) / (r.rows * r.D[:, None] ** 2)
    slack = 1e-12 * r.dx.abs() + abs(g) * 2.0 ** -50 * (F + 1.0 / (r.rows * r.n))
    assert ((xd.grad - r.dx).abs() <= slack).all(), ((xd.grad - r.dx).abs() / slack).max()


# mutant -> the case that must notice it (and whether in bf16)
MUTANTS = {
    "tail": ("1-normal", False),
    "trip2": ("3-soft", False),
    "no_nr": ("6-empty-15", False),
    "no_dr": ("6-empty-30", False),
    "one_over_n": ("1-normal", False),
    "no_rows": ("1-normal", False),
    "no_half": ("1-normal", False),
    "no_gout": ("3-soft", False),
    "p_not_pq": ("1-normal", False),
    "threshold": ("3-soft", False),
    "truncate": ("1-normal", True),
}


@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_mutant_is_rejected(mut):
    cid, bf16 = MUTANTS[mut]
    x, t, g, r, tol = _prepared(cid, bf16)
    rat = lr.ratios(r, tol, emulate(x, t, g, bf16=bf16, mut=mut))
    print(mut, "on", cid, {k: float(f"{v:.3g}") for k, v in rat.items()})
    assert any(not v <= 1.0 for v in rat.values()), f"no bound of case {cid} notices the mutant {mut}"
    caught = []
    for c in lr.SMALL:
        x, t, g, r, tol = _prepared(c, bf16)
        if any(not v <= 1.0 for v in lr.ratios(r, tol, emulate(x, t, g, bf16=bf16, mut=mut)).values()):
            caught.append(c)
    print(mut, "caught on", caught)


def test_loop_cases_notice_a_dropped_trip_and_a_dropped_tail():
    """the loop cases of either kernel: a dropped second trip and a dropped last element move the sums and the gradient past their bounds"""
    for cid in lr.LOOP:
        x, t, g, r, tol = _prepared(cid)
        for mut in ("trip2", "tail"):
            rat = lr.ratios(r, tol, emulate(x, t, g, mut=mut))
            assert not rat["sums"] <= 1.0 and not rat["dx"] <= 1.0, (cid, mut, rat)
