"""The definition of "correct" for the InstanceNorm + LeakyReLU kernels of csrc/norm.hip: a float64 reference written out by hand,
the bounds a correct kernel has to meet, and the input cases shared by tests/test_norm_ref.py (CPU: proves reference and bounds on an
emulation of the kernels' arithmetic) and tests/test_norm_gpu.py (the kernels themselves). Plain torch, any device, no native code.

Layout here is always [B][n][C] (n = H * W pixels); `bnc()` brings NHWC and NCHW tensors into it.

What a correct kernel may do, and what every coefficient below stands for:
  * per-thread partial sums in fp32 (at most ~16 terms each), folded in double       -> 2^-20 on the sums (STAT_BF16)
  * sums that come from a convolution's epilogue (fp32 over a whole tile)            -> 2^-16 (STAT_EPILOGUE; the 1e-5 the epilogue test grants)
  * the NCHW fp32 kernels accumulate in double                                       -> 2^-40 (STAT_F32)
  * mean and rstd are rounded to fp32                                                -> 2^-23 |mean|, 2^-22 (rstd: rounding + sqrt + division)
  * fp32 elementwise arithmetic in any order, fused or not                           -> 2^-16 of the largest operand (256 fp32 ulps; 2^-20 for
                                                                                        fp32 outputs), far below bf16 resolution
  * ONE rounding to bf16                                                             -> 2^-8 |ref|, half a bf16 ulp
  * fp32 sums of the gradients (dgamma, dbeta, dhead)                                -> 2^-19 of the sum of magnitudes
  * the branch z > 0 is taken in fp32: elements with |z| <= 2^-15 T + dz (`near`) are left out of the elementwise comparisons, their
    possible effect on the sums is added to the bounds, and they may be at most NEAR_CAP = 0.2 % of a case (a condition on the inputs).
"""
from types import SimpleNamespace

import torch

STAT_BF16, STAT_EPILOGUE, STAT_F32 = 2.0 ** -20, 2.0 ** -16, 2.0 ** -40
NEAR_CAP = 0.002
EPS = 1e-5


def bnc(t, layout):
    """[B,H,W,C] ("nhwc") or [B,C,H,W] ("nchw") -> [B][n][C] view"""
    if layout == "nhwc":
        return t.reshape(t.shape[0], -1, t.shape[-1])
    return t.reshape(t.shape[0], t.shape[1], -1).transpose(1, 2)


def reference(x, w, b, slope, eps=EPS, dy=None, head_w=None, head_b=None, dlogit=None):
    """x [B][n][C] (the very bf16 / fp32 values the kernel gets), w / b [C] or None, dy like x, head_w [C], head_b [1] or None, dlogit [B][n].
    Everything in float64, by the formulas of the operation (not F.instance_norm: that refuses n = 1)."""
    x = x.double()
    B, n, C = x.shape
    wd = w.double() if w is not None else torch.ones(C, dtype=torch.float64, device=x.device)
    bd = b.double() if b is not None else torch.zeros(C, dtype=torch.float64, device=x.device)
    r = SimpleNamespace(x=x, n=n, w=wd, b=bd, slope=float(slope), eps=float(eps))
    r.mean = x.sum(1) / n
    r.ex2 = (x * x).sum(1) / n
    r.eabs = x.abs().sum(1) / n
    r.var = (r.ex2 - r.mean * r.mean).clamp_min(0)
    r.rstd = 1.0 / torch.sqrt(r.var + eps)
    r.xh = (x - r.mean[:, None]) * r.rstd[:, None]
    r.z = r.xh * wd + bd
    r.pos = r.z > 0
    r.y = torch.where(r.pos, r.z, slope * r.z)
    r.scale = wd * r.rstd
    r.shift = bd - r.mean * r.scale
    if head_w is not None:
        r.hw = head_w.double().reshape(C)
        r.logits = (r.y * r.hw).sum(2) + (head_b.double().reshape(()) if head_b is not None else 0.0)
        if dlogit is not None:
            r.dl = dlogit.double().reshape(B, n)
            dy = r.dl[:, :, None] * r.hw
            r.dhead_w = (r.y * r.dl[:, :, None]).sum((0, 1))
            r.dhead_b = r.dl.sum().reshape(1)
    if dy is not None:
        r.dy = dy.double()
        r.g = torch.where(r.pos, r.dy, slope * r.dy)
        r.mg = r.g.sum(1) / n
        r.mgx = (r.g * r.xh).sum(1) / n
        r.dx = r.scale[:, None] * (r.g - r.mg[:, None] - r.xh * r.mgx[:, None])
        r.dgamma = (r.g * r.xh).sum((0, 1))
        r.dbeta = r.g.sum((0, 1))
    return r


def bounds(r, stat=STAT_BF16, f32=False):
    """Tolerance per output of reference r (same names), plus `near` and its share. stat: the coefficient of the sums (module constants);
    f32: fp32 outputs (no bf16 rounding, 2^-20 operand term, the forward subtracts the mean first)."""
    half_ulp, op = (0.0, 2.0 ** -20) if f32 else (2.0 ** -8, 2.0 ** -16)
    t = SimpleNamespace()
    t.rho = stat * r.ex2 / (r.var + r.eps) + 2.0 ** -22             # |d rstd| / rstd
    t.mu = stat * r.eabs + 2.0 ** -23 * r.mean.abs()                 # |d mean|
    s = r.w.abs() * r.rstd                                           # [B][C]
    t.mean, t.rstd = t.mu, t.rho * r.rstd
    t.scale = s * t.rho                                              # rho's 2^-22 holds the roundings of rstd and of w * rstd (2^-24 each)
    # shift = b - mean * scale: the shift of z at x = 0, and the final subtraction rounds once (half an fp32 ulp of a result <= |b| + |mean * scale|;
    # the second part is within rho's 2^-22 already)
    t.shift = s * (r.mean.abs() * t.rho + t.mu) + 2.0 ** -23 * r.b.abs()
    dev = (r.x - r.mean[:, None]).abs()
    t.dz = s[:, None] * (dev * t.rho[:, None] + t.mu[:, None])       # propagated shift of z
    T = (dev if f32 else r.x.abs() + r.mean.abs()[:, None]) * s[:, None] + r.b.abs()
    if r.slope == 1.0:
        t.near = torch.zeros_like(r.pos)                            # no branch
    else:
        t.near = r.z.abs() <= 2.0 ** -15 * T + t.dz
    t.near_share = t.near.double().mean().item()
    t.y = half_ulp * r.y.abs() + op * T + t.dz
    if hasattr(r, "logits"):
        t.logits = 2.0 ** -8 * r.logits.abs() + 2.0 ** -16 * (r.y * r.hw).abs().sum(2) + (r.hw.abs() * t.dz).sum(2)
    if hasattr(r, "dl"):
        t.dhead_w = 2.0 ** -19 * (r.y * r.dl[:, :, None]).abs().sum((0, 1)) + (t.dz * r.dl.abs()[:, :, None]).sum((0, 1))
        t.dhead_b = 2.0 ** -19 * r.dl.abs().sum().reshape(1)
    if hasattr(r, "dy"):
        k = 1.0 - r.slope
        sn_dy = (t.near * r.dy.abs()).sum(1)                        # [B][C]: what the borderline elements can move in sum g ...
        sn_dyx = (t.near * (r.dy * r.xh).abs()).sum(1)              # ... and in sum g * xh
        F = s[:, None] * (k * sn_dy[:, None] / r.n + r.xh.abs() * k * sn_dyx[:, None] / r.n)
        D = s[:, None] * (r.g.abs() + r.mg.abs()[:, None] + (r.xh * r.mgx[:, None]).abs())
        t.dx = half_ulp * r.dx.abs() + op * D + 3.0 * t.rho[:, None] * D + F
        gx = (r.g * r.xh).abs()
        t.dgamma = 2.0 ** -19 * gx.sum((0, 1)) + (2.0 * t.rho[:, None] * gx + r.g.abs() * (r.rstd * t.mu)[:, None]).sum((0, 1)) + k * sn_dyx.sum(0)
        t.dbeta = 2.0 ** -19 * r.g.abs().sum((0, 1)) + k * sn_dy.sum(0)
    return t


ELEMENTWISE = ("y", "dx")       # compared outside `near` only


def ratios(r, t, got):
    """got: name -> tensor in r's layout ([B][n][C] for y / dx, [B][n] logits, [B][C] statistics, [C] gradients). Returns name -> the largest
    error / bound; an error where the bound is 0 counts as inf. Asserts the `near` condition of the case."""
    assert t.near_share <= NEAR_CAP, f"near holds {t.near_share:.4%} of the case: change the case's inputs, not the cap"
    out = {}
    for name, v in got.items():
        want, tol = getattr(r, name), getattr(t, name)
        v = v.double().reshape(want.shape)
        err = (v - want).abs()
        if name in ELEMENTWISE:
            err = torch.where(t.near, torch.zeros_like(err), err)
        q = torch.where(err == 0, torch.zeros_like(err), err / tol)           # err > 0 over tol == 0 -> inf
        q = torch.where(torch.isnan(v), torch.full_like(q, float("inf")), q)
        out[name] = q.max().item() if q.numel() else 0.0
    return out


def assert_within(rat, what=""):
    bad = {k: v for k, v in rat.items() if not v <= 1.0}
    assert not bad, f"{what}: error / bound above 1 for {bad} (all: {rat})"


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# Inputs are drawn on the CPU from a generator seeded per case, so that the CPU proof and the GPU test see the same numbers.

# id: (B, H, W, C, affine, slope, off, sd)
NHWC_CASES = {
    1: (2, 37, 53, 32, "wb", 0.01, 0.7, 2.0),
    2: (1, 1, 1, 8, "wb", 0.01, 0.3, 1.0),
    3: (3, 1, 3, 24, "", 0.0, 0.0, 1.0),
    4: (1, 5, 17, 40, "w", 0.2, 0.2, 1.0),
    5: (2, 1, 127, 16, "b", 0.01, 0.0, 1.0),
    6: (2, 1, 129, 16, "", 1.0, 0.0, 1.0),
    7: (1, 255, 257, 8, "wb", 0.01, 0.7, 2.0),
    8: (1, 256, 256, 8, "", 0.2, 0.0, 1.0),
    9: (1, 256, 257, 8, "wb", 0.01, 0.0, 1.0),
    10: (1, 9, 7, 512, "wb", 0.01, 0.1, 1.0),
    11: (2, 19, 23, 256, "", 0.0, 0.0, 1.0),
    12: (2, 37, 53, 32, "wb", 0.01, 8.0, 1.0),
    13: (2, 37, 53, 32, "wb", 0.01, 0.7, 2.0),
}


def _affine(gen, C, affine, n, min_b=0.0):
    w = torch.rand(C, generator=gen) + 0.5
    b = 0.5 * torch.randn(C, generator=gen)
    if n == 1:
        min_b = 0.25        # a one-pixel plane has z = b exactly: keep b clear of the borderline band (2^-15 T is ~0.1 at rstd = eps^-1/2)
    if min_b:
        b = torch.where(b < 0, -b.abs().clamp_min(min_b), b.abs().clamp_min(min_b))
    return (w if "w" in affine else None), (b if "b" in affine else None)


def nhwc_case(cid, device="cpu"):
    """-> x [B,H,W,C] bf16, dy like x, w, b (fp32 or None), slope"""
    B, H, W, C, affine, slope, off, sd = NHWC_CASES[cid]
    gen = torch.Generator().manual_seed(7000 + cid)
    x = (torch.randn(B, H, W, C, generator=gen) * sd + off).to(torch.bfloat16)
    if cid == 13:
        x[..., 5] = 0.69921875          # exact in bf16: a constant channel, var = 0
    dy = torch.randn(B, H, W, C, generator=gen).to(torch.bfloat16)
    w, b = _affine(gen, C, affine, H * W, min_b=0.1 if cid == 13 else 0.0)
    mv = lambda t: t.to(device) if t is not None else None
    return mv(x), mv(dy), mv(w), mv(b), slope


HEAD_GEOMETRIES = [(c, b, h, w) for c in (8, 16, 128, 256) for (b, h, w) in ((1, 1, 1), (3, 7, 9), (1, 1, 257), (2, 37, 53))]
HEAD_VARIANTS = ("affine", "plain")       # slope 0.01 with affine and head bias; no affine, no head bias, slope 0.2


def head_case(C, B, H, W, variant, device="cpu"):
    """-> x, dlogit [B,H,W,1] bf16, w, b, head_w [1,C,1,1], head_b [1] or None, slope"""
    gen = torch.Generator().manual_seed(9000 + C * 7 + B * 131 + H * W + (variant == "plain"))
    x = (torch.randn(B, H, W, C, generator=gen) + 0.3).to(torch.bfloat16)
    dl = torch.randn(B, H, W, 1, generator=gen).to(torch.bfloat16)
    w, b = _affine(gen, C, "wb" if variant == "affine" else "", H * W)
    hw = torch.randn(1, C, 1, 1, generator=gen) / C ** 0.5
    hb = torch.randn(1, generator=gen) if variant == "affine" else None
    mv = lambda t: t.to(device) if t is not None else None
    return mv(x), mv(dl), mv(w), mv(b), mv(hw), mv(hb), (0.01 if variant == "affine" else 0.2)


def _nchw_cases():
    out, k = [], 0
    affines, slopes = ("wb", "", "w"), (0.0, 0.01, 1.0)
    for n in (1, 3, 7, 8, 2047, 2048, 3 * 2048 + 5):
        for planes in (1, 5):
            for dt in ("f32", "bf16"):
                # every (affine, slope) pair comes up: k walks the 3 x 3 grid. A one-pixel plane has z = b exactly, so it takes the
                # affine form that has a b (without one every element is borderline by construction)
                a, s = affines[k % 3], slopes[(k // 3) % 3]
                out.append((n, planes, dt, "wb" if n == 1 else a, s, "randn"))
                k += 1
    out.append((2047, 5, "f32", "wb", 0.01, "flat"))        # x = 100 + 0.01 randn: the nearly constant channel the double accumulation is for
    return out


NCHW_CASES = _nchw_cases()


def nchw_case(case, device="cpu"):
    """-> x [B,C,1,n], dy, w, b, slope with B * C = planes (5 planes: B = 1, C = 5)"""
    n, planes, dt, affine, slope, kind = case
    gen = torch.Generator().manual_seed(11000 + n * 3 + planes + (dt == "f32") * 17 + (kind == "flat") * 5)
    x = torch.randn(1, planes, 1, n, generator=gen)
    x = 100.0 + 0.01 * x if kind == "flat" else x * 1.5 + 0.4
    dy = torch.randn(1, planes, 1, n, generator=gen)
    dtype = torch.float32 if dt == "f32" else torch.bfloat16
    w, b = _affine(gen, planes, affine, n)
    mv = lambda t: t.to(device) if t is not None else None
    return mv(x.to(dtype)), mv(dy.to(dtype)), mv(w), mv(b), slope


def split_sums(x, nslot, gen):
    """The exact fp64 (sum x, sum x^2) of x [B][n][C], split at random over nslot slots, some parts negative -> [nslot][B][C][2] float64"""
    xd = x.double().cpu()
    tot = torch.stack((xd.sum(1), (xd * xd).sum(1)), dim=-1)          # [B][C][2]
    wts = torch.randn((nslot,) + tuple(tot.shape), generator=gen, dtype=torch.float64)
    wts = wts - wts.mean(0, keepdim=True) + 1.0 / nslot               # sums to 1 over the slots, of either sign
    parts = wts * tot
    parts[0] += tot - parts.sum(0)                                    # what the split lost to rounding
    return parts
