"""Proves tests/_norm_ref.py without a GPU: an emulation of the arithmetic of csrc/norm.hip in torch on the CPU (fp32 partial sums folded in
double, fp32 mean / rstd, x * g + sh forward, (x - mean) * rstd * w + b branch decision in backward, one rounding to bf16) stays inside
every bound on every case that tests/test_norm_gpu.py runs, and each of a list of wrong kernels (mutants of the emulation) breaks at
least one bound on at least one case. This is the evidence that the GPU tests can pass for a right kernel and fail for a wrong one."""
import functools

import pytest
import torch

import _norm_ref as nr

MUTANTS = ("last_pixel", "unbiased", "no_eps", "slope", "no_xh_mgx", "swap", "first_slot")


def _sum32(v):
    """sum over dim 1 of a float32 [B][n]... as a kernel forms it: running fp32 sums of 16 terms each, folded in double"""
    B, n = v.shape[:2]
    pad = (-n) % 16
    if pad:
        v = torch.cat((v, v.new_zeros((B, pad) + tuple(v.shape[2:]))), dim=1)
    v = v.reshape((B, -1, 16) + tuple(v.shape[2:]))
    acc = v[:, :, 0].clone()
    for i in range(1, 16):          # torch.sum / cumsum would accumulate in double on the CPU
        acc = acc + v[:, :, i]
    return acc.double().sum(1)


def emulate(x, w, b, slope, eps=nr.EPS, dy=None, f32=False, head=None, slots=None, mut=None):
    """x, dy [B][n][C]; head = (head_w [C], head_b or None, dlogit [B][n] or None); slots [nslot][B][C][2] float64. -> name -> tensor"""
    xf = x.float()
    B, n, C = xf.shape
    if slots is not None:
        tot = slots[0] if mut == "first_slot" else slots.sum(0)
        a, q = tot[..., 0], tot[..., 1]
    else:
        xs = xf[:, :-1] if mut == "last_pixel" else xf
        if f32:
            a, q = xs.double().sum(1), (xs.double() * xs.double()).sum(1)
        else:
            a, q = _sum32(xs), _sum32(xs * xs)
    mean_d = a / n
    var = q / n - mean_d * mean_d
    if mut == "unbiased" and n > 1:
        var = var * n / (n - 1)
    var = var.clamp_min(0)
    rstd = (1.0 / torch.sqrt(var + (0.0 if mut == "no_eps" else float(torch.tensor(eps, dtype=torch.float32))))).float()
    mean = mean_d.float()
    wc = w.float() if w is not None else torch.ones(C)
    bc = b.float() if b is not None else torch.zeros(C)
    sl = torch.tensor(slope * 0.5 + 0.03 if mut == "slope" else slope, dtype=torch.float32)
    g = wc * rstd if w is not None else rstd
    sh = bc - mean * g
    z = (xf - mean[:, None]) * g[:, None] + bc if f32 else xf * g[:, None] + sh[:, None]
    y = torch.where(z > 0, z, z * sl)
    out = dict(mean=mean, rstd=rstd, scale=g, shift=sh)
    if head is None:
        out["y"] = y if f32 else y.bfloat16()
    else:
        hv, hb, dl = head
        hv = hv.float().reshape(C)
        part = (y * hv).reshape(B, n, C // 8, 8)
        dot = part[..., 0].clone()
        for k in range(1, 8):
            dot = dot + part[..., k]
        lg = dot[..., 0].clone()
        for k in range(1, C // 8):
            lg = lg + dot[..., k]
        out["logits"] = (lg + (hb.float().reshape(()) if hb is not None else 0.0)).bfloat16()
        if dl is not None:
            dlf = dl.float().reshape(B, n)
            dy = dlf[:, :, None] * hv
    if dy is None:
        return out
    d = dy.float()
    xh = (xf - mean[:, None]) * rstd[:, None]
    pre = xh * wc + bc
    gk = torch.where(pre > 0, d, d * sl)
    sa, sq = _sum32(gk), _sum32(gk * xh)
    mg, mgx = (sa / n).float(), (sq / n).float()
    k0 = (wc * rstd)[:, None]
    dx = k0 * (gk - mg[:, None]) if mut == "no_xh_mgx" else k0 * (gk - mg[:, None] - xh * mgx[:, None])
    out["dx"] = dx if f32 else dx.bfloat16()
    dgamma, dbeta = sq.sum(0).float(), sa.sum(0).float()
    out["dgamma"], out["dbeta"] = (dbeta, dgamma) if mut == "swap" else (dgamma, dbeta)
    if head is not None and head[2] is not None:
        ya = torch.where(pre > 0, pre, pre * sl)
        out["dhead_w"] = _sum32(ya * dlf[:, :, None]).sum(0).float()
        out["dhead_b"] = _sum32(dlf).sum().float().reshape(1)
    return out


# ---- the cases, each with its reference and bounds computed once ---------------------------------------------------------------------

def _names():
    for cid in nr.NHWC_CASES:
        yield ("nhwc", cid)
    for cid in (1, 4):
        yield ("slots", cid)
    for geo in nr.HEAD_GEOMETRIES:
        for v in nr.HEAD_VARIANTS:
            yield ("head",) + geo + (v,)
    for c in nr.NCHW_CASES:
        yield ("nchw",) + c


ALL = list(_names())


@functools.lru_cache(maxsize=None)
def _prepared(name):
    """-> (emulate kwargs, reference, bounds)"""
    kind = name[0]
    if kind in ("nhwc", "slots"):
        x, dy, w, b, slope = nr.nhwc_case(name[1])
        x, dy = nr.bnc(x, "nhwc"), nr.bnc(dy, "nhwc")
        kw = dict(x=x, w=w, b=b, slope=slope, dy=dy)
        if kind == "slots":
            kw["slots"] = nr.split_sums(x, 9, torch.Generator().manual_seed(5))
        r = nr.reference(x, w, b, slope, dy=dy)
        return kw, r, nr.bounds(r)
    if kind == "head":
        x, dl, w, b, hw, hb, slope = nr.head_case(*name[1:])
        x = nr.bnc(x, "nhwc")
        kw = dict(x=x, w=w, b=b, slope=slope, head=(hw, hb, dl))
        r = nr.reference(x, w, b, slope, head_w=hw, head_b=hb, dlogit=dl)
        return kw, r, nr.bounds(r)
    x, dy, w, b, slope = nr.nchw_case(name[1:])
    f32 = x.dtype == torch.float32
    x, dy = nr.bnc(x, "nchw"), nr.bnc(dy, "nchw")
    r = nr.reference(x, w, b, slope, dy=dy)
    return dict(x=x, w=w, b=b, slope=slope, dy=dy, f32=f32), r, nr.bounds(r, stat=nr.STAT_F32 if f32 else nr.STAT_BF16, f32=f32)


def _forced(name):
    """A one-pixel plane without affine has z = 0 on every element: all of it is `near` by construction, whatever the inputs, and
    nothing is left to bound. tests/test_norm_gpu.py asserts the values the arithmetic forces there instead."""
    return name[0] == "head" and name[3] * name[4] == 1 and name[5] == "plain"


def test_near_condition_holds_on_every_case():
    worst = 0.0
    for name in ALL:
        if _forced(name):
            continue
        _, r, t = _prepared(name)
        assert t.near_share <= nr.NEAR_CAP, (name, t.near_share)
        if r.slope == 1.0:
            assert not t.near.any()
        worst = max(worst, t.near_share)
    print(f"largest share of borderline elements: {worst:.4%}")


@pytest.mark.parametrize("kind", ["nhwc", "slots", "head", "nchw"])
def test_emulated_kernel_is_within_every_bound(kind):
    worst = {}
    for name in ALL:
        if name[0] != kind or _forced(name):
            continue
        kw, r, t = _prepared(name)
        rat = nr.ratios(r, t, emulate(**kw))
        nr.assert_within(rat, str(name))
        for k, v in rat.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(kind, {k: round(v, 4) for k, v in worst.items()})
    assert worst


def test_forced_one_pixel_case_is_all_borderline():
    for name in ALL:
        if _forced(name):
            _, r, t = _prepared(name)
            assert t.near.all() and (r.z == 0).all() and (r.dx == 0).all() and (r.logits == 0).all()


@pytest.mark.parametrize("mut", MUTANTS)
def test_mutant_is_rejected(mut):
    """each wrong kernel breaks a bound somewhere on the cases of the plain channels-last family (the slot mutant: on the slot cases)"""
    caught = []
    for name in ALL:
        if name[0] != ("slots" if mut == "first_slot" else "nhwc"):
            continue
        kw, r, t = _prepared(name)
        rat = nr.ratios(r, t, emulate(mut=mut, **kw))
        if any(not v <= 1.0 for v in rat.values()):
            caught.append((name[1], max(rat, key=lambda k: rat[k] if rat[k] == rat[k] else float("inf"))))
    print(mut, "caught on", len(caught), "cases:", caught)
    assert caught, f"no bound notices the mutant {mut}"


def test_exact_zeros_of_the_one_pixel_plane():
    """case 2 (n = 1): var = 0, rstd = eps^-1/2, and dx / dgamma are exactly 0 in the reference and in the emulation"""
    kw, r, _ = _prepared(("nhwc", 2))
    got = emulate(**kw)
    assert (r.var == 0).all() and (r.dx == 0).all() and (r.dgamma == 0).all()
    assert (got["dx"].float() == 0).all() and (got["dgamma"] == 0).all()
    assert torch.allclose(got["rstd"].double(), torch.full_like(r.rstd, nr.EPS ** -0.5), rtol=1e-6)
