"""The definition of "correct" for the fused Dice + BCE loss of csrc/loss.hip: a float64 reference written out by hand, the bounds a
correct kernel has to meet, and the input cases shared by tests/test_loss_ref.py (CPU: proves reference and bounds on an emulation of
the kernels' arithmetic) and tests/test_loss_gpu.py (the kernels themselves). Plain torch, any device, no native code.

Layout here is always [rows][n]: one row per (sample, channel) plane, which is what the entry points take.

    p = sigmoid(x), e = exp(-|x|)
    S0 = sum p t, S1 = sum p, S2 = sum t, S3 = sum max(x, 0) - x t + log1p(e)        per row
    N = 2 S0 + nr, D = S1 + S2 + dr
    loss = (mean_rows(1 - N / D) + sum_rows S3 / (rows n)) / 2
    dx = g / 2 * [A p (1 - p) + (p - t) / (rows n)],  A = -(2 t D - N) / (rows D^2)

What a correct kernel may do, with u = 2^-24 (the unit roundoff of fp32), a = |x|, and what every coefficient below stands for:
  * e = __expf(-a) = exp2(-a * L), L = fl(log2 e). L is off by at most half an ulp of [1, 2), 0.69 u relative, the product rounds once
    (u), and ln 2 * a * log2 e = a, so the argument costs 1.69 u a of relative error in e: C_A = 2. The hardware exp2 is good to one
    ulp = 2 u, and a lowering that scales the argument range multiplies once more and may be an ulp off again: C_E = 4. Results
    below 2^-126 may be flushed to zero: FLOOR = 2^-125 absolute.                                        de / e <= (C_E + C_A a) u + FLOOR / e
  * p = 1 / (1 + e) or e / (1 + e): one sum, one division, and the rounding of e where it is the numerator: C_P = 3 u p; d p / d e =
    -+ p q / e. An ABSOLUTE error: 1 - p and p - t of a confident pixel keep no relative accuracy, as in any fp32 evaluation.
                                                                                                        dp <= C_P u p + p q de / e + FLOOR
  * terms: p t carries dp and one rounding; p carries dp; t is exact. The BCE term rounds x t, the difference and the last sum once each
    (the last one is counted with the sums), log1pf is given C_L = 3 u (two ulps of the function, one of its argument 1 + e), and
    d log1p(e) = e / (1 + e) * de / e.
  * sums: a thread chains K terms in fp32 (K - 1 additions of at most u of the running sum of magnitudes each), everything after that is
    double. C_S = 2 more: the rounding of the term itself before it is added, and one for the second-order terms and the double fold.
                                                                                                        dS <= sum dterm + (K + C_S) u sum |term|
    K = ceil(n / (gx * 256)) with gx from the entry point's grid rule (`grid_x` below: part of the kernel's contract).
  * loss: dS through 1 - N / D and S3 / (rows n) in float64, plus one fp32 rounding of the result.
  * gradient, with F = (2 t D + N) / (rows D^2) >= |A|:
      - C_G = 8 u F p q: the roundings of fD and fN (together one u of 2 t D + N), of 2 t fD, of the difference, of kd, of the product
        with kd, of 1 - p, and of the two products with p and 1 - p;
      - F dp: the derivative of p (1 - p) is at most one;
      - dA p q, dA from dN and dD (the backward takes nr and dr as fp32: u nr, u dr more);
      - (dp + u (p + t) + 2 u |p - t|) / (rows n): the difference, the rounding of 1 / (rows n), the product;
      - 2 u |dx|: the last sum and the product with g / 2 (g / 2 itself is exact);
      - FLOOR: a result in the denormal range may be flushed (and bf16 has the exponent range of fp32: its denormals are 2^-133 apart);
      - bf16 output: ONE rounding, 2^-8 |dx|.
"""
from types import SimpleNamespace

import torch

U = 2.0 ** -24
C_E, C_A, C_P, C_L, C_S, C_G = 4.0, 2.0, 3.0, 3.0, 2.0, 8.0
FLOOR = 2.0 ** -125
NR = DR = 1e-5
CUS = 256                # an MI355X; the GPU tests ask the device
G = 0.37


def grid_x(n, rows, cus, kernel):
    """blocks along a row: ceil(n / 2048), capped by ceil(4 CUs / rows) forward and ceil(8 CUs / rows) backward, at least 1"""
    cap = ((4 if kernel == "fwd" else 8) * cus + rows - 1) // rows
    return max(1, min((n + 2047) // 2048, cap))


def trips(n, rows, cus, kernel):
    """K: how many elements one thread takes"""
    return -(-n // (grid_x(n, rows, cus, kernel) * 256))


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def reference(x, t, gout, smooth_nr=NR, smooth_dr=DR):
    """x, t [rows][n] (x: the very fp32 / bf16 values the kernel gets), gout: the upstream gradient as the kernel gets it (an fp32 value)"""
    x, t = x.double(), t.double()
    rows, n = x.shape
    r = SimpleNamespace(x=x, t=t, rows=rows, n=n, g=float(gout), nr=float(smooth_nr), dr=float(smooth_dr))
    r.a = x.abs()
    r.e = torch.exp(-r.a)
    big, small = 1.0 / (1.0 + r.e), r.e / (1.0 + r.e)
    r.p = torch.where(x >= 0, big, small)
    r.q = torch.where(x >= 0, small, big)               # 1 - p without cancellation
    r.bce = x.clamp_min(0) - x * t + torch.log1p(r.e)
    r.sums = torch.stack(((r.p * t).sum(1), r.p.sum(1), t.sum(1), r.bce.sum(1)), 1)
    r.N = 2.0 * r.sums[:, 0] + r.nr
    r.D = r.sums[:, 1] + r.sums[:, 2] + r.dr
    r.loss = ((1.0 - r.N / r.D).mean() + r.sums[:, 3].sum() / (rows * n)) / 2.0
    N, D = r.N[:, None], r.D[:, None]
    r.A = -(2.0 * t * D - N) / (rows * D * D)
    r.dx = r.g / 2.0 * (r.A * r.p * r.q + (r.p - t) / (rows * n))
    return r


def bounds(r, K, bf16=False):
    """-> tolerances `sums` [rows][4], `loss`, `dx` [rows][n]; K from trips() of the forward kernel"""
    x, t, p, q, e = r.x, r.t, r.p, r.q, r.e
    rn = r.rows * r.n
    re = (C_E + C_A * r.a) * U + FLOOR / e.clamp_min(1e-300)
    dp = C_P * U * p + p * q * re + FLOOR
    xt, dif, l1p = (x * t).abs(), (x.clamp_min(0) - x * t).abs(), torch.log1p(e)
    terms = (p * t, p, t, dif + l1p)
    dterm = (t * dp + U * p * t, dp, torch.zeros_like(p), U * (xt + dif) + C_L * U * l1p + e / (1.0 + e) * re)
    tol = SimpleNamespace(dp=dp)
    tol.sums = torch.stack([d.sum(1) + (K + C_S) * U * m.sum(1) for d, m in zip(dterm, terms)], 1)
    dN, dD = 2.0 * tol.sums[:, 0], tol.sums[:, 1] + tol.sums[:, 2]
    tol.loss = ((dN / r.D + r.N / r.D ** 2 * dD).mean() + tol.sums[:, 3].sum() / rn) / 2.0 + U * r.loss.abs()
    dN, dD = (dN + U * r.nr)[:, None], (dD + U * r.dr)[:, None]
    N, D = r.N[:, None], r.D[:, None]
    kd = 1.0 / (r.rows * D * D)
    F = (2.0 * t * D + N) * kd
    dA = (2.0 * t * dD + dN) * kd + r.A.abs() * 2.0 * dD / D
    tol.dx = abs(r.g) / 2.0 * (C_G * U * F * p * q + F * dp + dA * p * q + (dp + U * (p + t) + 2.0 * U * (p - t).abs()) / rn) + 2.0 * U * r.dx.abs() + FLOOR
    if bf16:
        tol.dx = tol.dx + 2.0 ** -8 * r.dx.abs()
    return tol


def ratios(r, tol, got):
    """got: name (sums, loss, dx) -> tensor. Returns name -> the largest error / bound; an error where the bound is 0, or a NaN, counts as inf."""
    out = {}
    for name, v in got.items():
        want, b = getattr(r, name), getattr(tol, name)
        v = v.double().reshape(want.shape)
        err = (v - want).abs()
        quo = torch.where(err == 0, torch.zeros_like(err), err / b)
        quo = torch.where(torch.isnan(v), torch.full_like(quo, float("inf")), quo)
        out[name] = quo.max().item()
    return out


def assert_within(rat, what=""):
    bad = {k: v for k, v in rat.items() if not v <= 1.0}
    assert not bad, f"{what}: error / bound above 1 for {bad} (all: {rat})"


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
# Inputs are drawn on the CPU from a generator seeded per case, so that the CPU proof and the GPU test see the same numbers. Every row
# ends in a distinctive element (logit +3, label 1) and holds the same at index 300 and at index 1100 where it is that long, so that a
# dropped tail or a dropped loop trip (the second trip starts at 256 with one block per row, at 1024 with four) moves every sum. In a
# row whose labels are all zero the distinctive elements keep label 0 and sit 6 above the row's mean logit: the sums stay as small as the
# case wants them, and the element still holds several per cent of them.

# id: (rows, n, kind, upstream gradient); rows may be a function of the CU count
CASES = {
    "1-normal": (3, 301, "normal", 1.0),
    "2-short": (2, 130, "normal", G),
    "2-single": (1, 1, "normal", G),
    "3-soft": (2, 999, "soft", G),
    "4-wide": (2, 777, "wide", G),
    "5-empty-row": (2, 1000, "empty0", G),
    "6-empty-15": (2, 1000, "empty-15", G),
    "6-empty-30": (2, 1000, "empty-30", G),
    "7-full+15": (2, 1000, "full+15", G),
    "8-fwd-trips": (lambda cus: 4 * cus + 1, 2350, "normal", G),
    "8-bwd-trips": (lambda cus: 8 * cus + 1, 2350, "normal", G),
    "8-fwd-cap": (lambda cus: cus + 44, 5 * 2048 + 77, "normal", G),
    "8-bwd-cap": (lambda cus: 2 * cus + 44, 5 * 2048 + 77, "normal", G),
}
SMALL = [c for c in CASES if not c.startswith("8")]
LOOP = [c for c in CASES if c.startswith("8")]


def case(cid, cus=CUS, device="cpu", bf16=False):
    """-> x [rows][n] fp32 (bf16: rounded to bf16 first, still held as the dtype the kernel gets), t [rows][n] fp32, gout (an fp32 value)"""
    rows, n, kind, g = CASES[cid]
    rows = rows(cus) if callable(rows) else rows
    gen = torch.Generator().manual_seed(3000 + sorted(CASES).index(cid))
    mean, sd = {"wide": (0.0, 40.0), "empty-15": (-15.0, 2.0), "empty-30": (-30.0, 2.0), "full+15": (15.0, 2.0)}.get(kind, (0.0, 3.0))
    x = torch.randn(rows, n, generator=gen) * sd + mean
    if kind == "soft":
        t = torch.rand(rows, n, generator=gen)
    else:
        t = (torch.rand(rows, n, generator=gen) > 0.8).float()
    if kind.startswith("empty-"):
        t.zero_()
    elif kind == "empty0":
        t[0].zero_()
    elif kind == "full+15":
        t.fill_(1.0)
    for i in {n - 1} | {j for j in (300, 1100) if j < n}:
        empty = t.sum(1) == 0 if kind.startswith("empty") else torch.zeros(rows, dtype=torch.bool)
        x[:, i] = torch.where(empty, torch.full((rows,), mean + 6.0), torch.full((rows,), 3.0))
        t[:, i] = torch.where(empty, torch.zeros(rows), torch.ones(rows))
    if cid == "8-fwd-trips":
        assert grid_x(n, rows, cus, "fwd") == 1 and trips(n, rows, cus, "fwd") >= 9 and n % 256
    if cid == "8-bwd-trips":
        assert grid_x(n, rows, cus, "bwd") == 1 and trips(n, rows, cus, "bwd") >= 9 and n % 256
    if cid.endswith("cap"):
        k = cid[2:5]
        assert 1 < grid_x(n, rows, cus, k) == ((4 if k == "fwd" else 8) * cus + rows - 1) // rows < (n + 2047) // 2048
    if bf16:
        x = x.to(torch.bfloat16)
    return x.to(device), t.to(device), f32(g)
