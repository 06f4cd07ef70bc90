"""The InstanceNorm + LeakyReLU kernels of csrc/norm.hip against the float64 reference and the derived bounds of tests/_norm_ref.py
(proved on the CPU by tests/test_norm_ref.py). Every test prints its error / bound ratios before it asserts them."""
import os
import subprocess
import sys

import pytest
import torch

import _norm_ref as nr

pytestmark = pytest.mark.gpu

EPS = nr.EPS
DEV = "cuda"


def _leaf(t):
    return t.clone().requires_grad_(True) if t is not None else None


def _report(what, rat):
    print("RATIO", what, {k: float(f"{v:.4g}") for k, v in rat.items()})
    nr.assert_within(rat, what)


def _grads(got, wm, bm):
    if wm is not None:
        got["dgamma"] = wm.grad
    if bm is not None:
        got["dbeta"] = bm.grad
    return got


def _eager(x, dy, w, b, slope, partials=None):
    """instance_norm_leaky_relu_nhwc through autograd -> the outputs by the names of the reference"""
    from octa_autosegmentation_amd.models import mfma_conv as mc
    xm, wm, bm = _leaf(x), _leaf(w), _leaf(b)
    y = mc.instance_norm_leaky_relu_nhwc(xm, wm, bm, slope, EPS, partials)
    assert y.dtype == torch.bfloat16 and y.shape == x.shape
    y.backward(dy)
    return _grads(dict(y=nr.bnc(y.detach(), "nhwc"), dx=nr.bnc(xm.grad, "nhwc")), wm, bm)


def _entry_fwd(x, w, b, slope, tiles=None, slots=None):
    """octa_instnorm_lrelu_nhwc_fwd with buffers of the test's own, as _InstNormLReLUNHWC.forward calls it -> y, mean, rstd"""
    from octa_autosegmentation_amd import _native
    B, C, hw = x.shape[0], x.shape[3], x.shape[1] * x.shape[2]
    y = torch.empty_like(x)
    mean, rstd = torch.empty(B * C, dtype=torch.float32, device=x.device), torch.empty(B * C, dtype=torch.float32, device=x.device)
    _native.launch("octa_instnorm_lrelu_nhwc_fwd", x.device, x, y, w, b, mean, rstd, B, C, hw, float(slope), EPS,
                   tiles, int(tiles.shape[1]) if tiles is not None else 0, slots, int(slots.shape[0]) if slots is not None else 0)
    return y, mean.view(B, C), rstd.view(B, C)


def _entry_both(x, dy, w, b, slope):
    """forward and backward entry points on the CALLING thread (autograd runs backward nodes on a thread of its own, which has another
    context), buffers as _InstNormLReLUNHWC lays them out -> the outputs by the names of the reference"""
    from octa_autosegmentation_amd import _native
    B, C, hw = x.shape[0], x.shape[3], x.shape[1] * x.shape[2]
    y, mean, rstd = _entry_fwd(x, w, b, slope)
    dx, dwb = torch.empty_like(x), torch.empty(2 * C, dtype=torch.float32, device=x.device)
    _native.launch("octa_instnorm_lrelu_nhwc_bwd", x.device, x, dy, w, b, mean, rstd, dx, dwb[:C], dwb[C:], B, C, hw, float(slope))
    return dict(y=nr.bnc(y, "nhwc"), dx=nr.bnc(dx, "nhwc"), mean=mean, rstd=rstd, dgamma=dwb[:C], dbeta=dwb[C:])


def _entry_head(x, dl, w, b, hw, hb, slope):
    """the fused head's two entry points on the calling thread, buffers as _InstNormLReLUHead1NHWC lays them out"""
    from octa_autosegmentation_amd import _native
    B, H, W, C = x.shape
    f32 = dict(dtype=torch.float32, device=x.device)
    hv = hw.reshape(-1).contiguous()
    mean, rstd = torch.empty(B * C, **f32), torch.empty(B * C, **f32)
    lg, dx = torch.empty((B, H, W, 1), dtype=torch.bfloat16, device=x.device), torch.empty_like(x)
    dgb, dhw, dhb = torch.empty(2 * C, **f32), torch.empty(C, **f32), torch.empty(1, **f32)
    _native.launch("octa_instnorm_lrelu_head1_nhwc_fwd", x.device, x, w, b, hv, hb, mean, rstd, lg, B, C, H * W, float(slope), EPS, None, 0)
    _native.launch("octa_instnorm_lrelu_head1_nhwc_bwd", x.device, x, dl, w, b, hv, mean, rstd, dx, dgb[:C], dgb[C:], dhw, dhb, B, C, H * W, float(slope))
    return dict(logits=lg.reshape(B, -1), dx=nr.bnc(dx, "nhwc"), mean=mean.view(B, C), rstd=rstd.view(B, C), dgamma=dgb[:C], dbeta=dgb[C:],
                dhead_w=dhw, dhead_b=dhb)


def _check_nhwc(what, x, dy, w, b, slope, partials=None, stat=nr.STAT_BF16):
    r = nr.reference(nr.bnc(x, "nhwc"), w, b, slope, EPS, dy=nr.bnc(dy, "nhwc"))
    t = nr.bounds(r, stat=stat)
    got = _eager(x, dy, w, b, slope, partials)
    tiles = partials if partials is not None and partials.dtype == torch.float32 else None
    slots = partials if partials is not None and partials.dtype == torch.float64 else None
    y2, got["mean"], got["rstd"] = _entry_fwd(x, w, b, slope, tiles, slots)
    _report(what, nr.ratios(r, t, got))
    _report(what + " (entry point)", nr.ratios(r, t, dict(y=nr.bnc(y2, "nhwc"))))
    return r, t, got


# ---- (a) own statistics pass ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", sorted(nr.NHWC_CASES))
def test_nhwc_forward_and_backward(hip_lib_built, cid):
    x, dy, w, b, slope = nr.nhwc_case(cid, DEV)
    r, t, got = _check_nhwc(f"nhwc case {cid}", x, dy, w, b, slope)
    if cid == 2:        # one pixel per plane: var = 0, and the gradient of a constant plane vanishes exactly
        assert (r.var == 0).all()
        assert torch.allclose(got["rstd"].double(), torch.full_like(r.rstd, EPS ** -0.5), rtol=1e-6)
        assert (got["dx"].float() == 0).all() and (got["dgamma"] == 0).all()
    if cid == 13:
        # the constant channel: no variance (the float64 reference may keep an ulp of it: 1e-16 against eps = 1e-5), rstd = eps^-1/2
        assert (r.var[:, 5] <= 1e-12).all()
        assert torch.allclose(got["rstd"].view(2, 32)[:, 5].double(), torch.full((2,), EPS ** -0.5, dtype=torch.float64, device=DEV), rtol=1e-6)


# ---- (b) statistics handed in --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nslot", [1, 7, 8, 9, 17, 1024])
@pytest.mark.parametrize("cid", [1, 4])
def test_nhwc_synthetic_slots(hip_lib_built, cid, nslot):
    x, dy, w, b, slope = nr.nhwc_case(cid, DEV)
    slots = nr.split_sums(nr.bnc(x, "nhwc"), nslot, torch.Generator().manual_seed(100 * cid + nslot)).to(DEV)
    assert slots.dtype == torch.float64 and (nslot == 1 or (slots < 0).any())
    _check_nhwc(f"slots case {cid} nslot {nslot}", x, dy, w, b, slope, partials=slots)


def _tile_partials(x, tiles, gen):
    """the exact sums of x [B][n][C] spread over `tiles` float32 partials of one sign [B][tiles][C][2] (their rounding: 2^-24 of the sum)"""
    xd = x.double().cpu()
    tot = torch.stack((xd.sum(1), (xd * xd).sum(1)), dim=-1)                    # [B][C][2]
    wts = torch.rand((x.shape[0], tiles, x.shape[2], 2), generator=gen, dtype=torch.float64) + 0.1
    wts = wts / wts.sum(1, keepdim=True)
    part = (wts * tot[:, None]).float()
    part[:, 0] += (tot - part.double().sum(1)).float()
    return part


@pytest.mark.parametrize("tiles", [1, 7, 8, 9, 100])
@pytest.mark.parametrize("cid", [1, 4])
def test_nhwc_synthetic_tiles(hip_lib_built, cid, tiles):
    x, dy, w, b, slope = nr.nhwc_case(cid, DEV)
    part = _tile_partials(nr.bnc(x, "nhwc"), tiles, torch.Generator().manual_seed(200 * cid + tiles)).to(DEV)
    assert part.dtype == torch.float32
    _check_nhwc(f"tiles case {cid} tiles {tiles}", x, dy, w, b, slope, partials=part, stat=nr.STAT_EPILOGUE)


@pytest.mark.parametrize("form", ["slots", "tiles"])
@pytest.mark.parametrize("h,w_", [(37, 45), (203, 70)])
def test_nhwc_statistics_from_the_convolution(hip_lib_built, h, w_, form):
    """the norm of the convolution's STORED bf16 result, with the statistics of its epilogue, against the float64 norm of that result"""
    from octa_autosegmentation_amd.models import mfma_conv as mc
    gen = torch.Generator().manual_seed(h * 7 + w_)
    xin = torch.randn(2, h, w_, 32, generator=gen).to(torch.bfloat16).to(DEV)
    wt = (torch.randn(64, 32, 3, 3, generator=gen) / (3.0 * 32 ** 0.5)).to(DEV)
    gam, bet = (torch.rand(64, generator=gen) + 0.5).to(DEV), (0.5 * torch.randn(64, generator=gen)).to(DEV)
    dy = torch.randn(2, h, w_, 64, generator=gen).to(torch.bfloat16).to(DEV)
    with torch.no_grad():
        y, part = mc.conv3x3(xin, wt, 1, form)
    assert part.dtype == (torch.float64 if form == "slots" else torch.float32)
    _check_nhwc(f"conv {h}x{w_} {form}", y, dy, gam, bet, 0.01, partials=part, stat=nr.STAT_EPILOGUE)


# ---- (c) lazy form -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", [1, 2, 3, 4, 5, 7])
def test_lazy_norm_and_materialise(hip_lib_built, cid):
    from octa_autosegmentation_amd.models import mfma_conv as mc
    x, dy, w, b, slope = nr.nhwc_case(cid, DEV)
    B, C = x.shape[0], x.shape[3]
    r = nr.reference(nr.bnc(x, "nhwc"), w, b, slope, EPS, dy=nr.bnc(dy, "nhwc"))
    t = nr.bounds(r)
    xm, wm, bm = _leaf(x), _leaf(w), _leaf(b)
    lazy = mc.lazy_norm(xm, wm, bm, slope, EPS)
    y = mc.materialise(lazy, slope)
    y.backward(dy)
    got = _grads(dict(scale=lazy[1].view(B, C), shift=lazy[2].view(B, C), y=nr.bnc(y.detach(), "nhwc"), dx=nr.bnc(xm.grad, "nhwc")), wm, bm)
    _report(f"lazy case {cid}", nr.ratios(r, t, got))
    if cid in (2, 3, 4, 5):     # one split: one addition into a zero, no ordering freedom -> the two forms are the same numbers
        eager = _eager(x, dy, w, b, slope)
        for k, v in eager.items():
            assert torch.equal(v, got[k]), (cid, k)


# ---- (d) fused norm + head -----------------------------------------------------------------------------------------------------------

def _head(x, dl, w, b, hw, hb, slope, partials=None):
    from octa_autosegmentation_amd import _native
    from octa_autosegmentation_amd.models import mfma_conv as mc
    xm, wm, bm, hwm, hbm = _leaf(x), _leaf(w), _leaf(b), _leaf(hw), _leaf(hb)
    lg = mc.instance_norm_leaky_relu_head1_nhwc(xm, wm, bm, slope, EPS, hwm, hbm, partials)
    assert lg.dtype == torch.bfloat16 and lg.shape == x.shape[:3] + (1,)
    lg.backward(dl)
    got = _grads(dict(logits=lg.detach().reshape(x.shape[0], -1), dx=nr.bnc(xm.grad, "nhwc"), dhead_w=hwm.grad.reshape(-1)), wm, bm)
    if hbm is not None:
        got["dhead_b"] = hbm.grad
    B, H, W, C = x.shape
    mean, rstd = torch.empty(B * C, dtype=torch.float32, device=x.device), torch.empty(B * C, dtype=torch.float32, device=x.device)
    lg2 = torch.empty_like(lg)
    _native.launch("octa_instnorm_lrelu_head1_nhwc_fwd", x.device, x, w, b, hw.reshape(-1).contiguous(), hb, mean, rstd, lg2, B, C, H * W,
                   float(slope), EPS, partials, int(partials.shape[0]) if partials is not None else 0)
    got["mean"], got["rstd"] = mean.view(B, C), rstd.view(B, C)
    return got


@pytest.mark.parametrize("variant", nr.HEAD_VARIANTS)
@pytest.mark.parametrize("C,B,H,W", nr.HEAD_GEOMETRIES)
def test_head_forward_and_backward(hip_lib_built, C, B, H, W, variant):
    x, dl, w, b, hw, hb, slope = nr.head_case(C, B, H, W, variant, DEV)
    got = _head(x, dl, w, b, hw, hb, slope)
    r = nr.reference(nr.bnc(x, "nhwc"), w, b, slope, EPS, head_w=hw, head_b=hb, dlogit=dl)
    if H * W == 1 and variant == "plain":
        # a one-pixel plane without affine: z = 0 on every element whatever the inputs, so all of the case is borderline and the bounds have
        # nothing to say; the arithmetic forces every value instead (x - mean = 0 exactly, and 0 times either slope is 0)
        assert (r.z == 0).all()
        assert (got["logits"].float() == 0).all() and (got["dx"].float() == 0).all() and (got["dhead_w"] == 0).all()
        assert torch.equal(got["mean"], x.float().reshape(B, C))
        assert torch.allclose(got["rstd"].double(), torch.full_like(r.rstd, EPS ** -0.5), rtol=1e-6)
        return
    _report(f"head C{C} B{B} {H}x{W} {variant}", nr.ratios(r, nr.bounds(r), got))


def test_head_with_statistics_handed_in(hip_lib_built):
    from octa_autosegmentation_amd.models import mfma_conv as mc
    # from the producing convolution, 32 -> 32
    gen = torch.Generator().manual_seed(77)
    xin = torch.randn(2, 37, 45, 32, generator=gen).to(torch.bfloat16).to(DEV)
    wt = (torch.randn(32, 32, 3, 3, generator=gen) / (3.0 * 32 ** 0.5)).to(DEV)
    with torch.no_grad():
        y, part = mc.conv3x3(xin, wt, 1, "slots")
    assert part.dtype == torch.float64
    _, dl, w, b, hw, hb, slope = nr.head_case(32, 2, 37, 45, "affine", DEV)
    got = _head(y, dl, w, b, hw, hb, slope, partials=part)
    r = nr.reference(nr.bnc(y, "nhwc"), w, b, slope, EPS, head_w=hw, head_b=hb, dlogit=dl)
    _report("head slots from conv", nr.ratios(r, nr.bounds(r, stat=nr.STAT_EPILOGUE), got))
    # synthetic, C = 8
    x, dl, w, b, hw, hb, slope = nr.head_case(8, 3, 7, 9, "affine", DEV)
    slots = nr.split_sums(nr.bnc(x, "nhwc"), 9, torch.Generator().manual_seed(78)).to(DEV)
    got = _head(x, dl, w, b, hw, hb, slope, partials=slots)
    r = nr.reference(nr.bnc(x, "nhwc"), w, b, slope, EPS, head_w=hw, head_b=hb, dlogit=dl)
    _report("head synthetic slots", nr.ratios(r, nr.bounds(r), got))


# ---- (e) NCHW, fp32 and bf16 ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", nr.NCHW_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_nchw_forward_and_backward(hip_lib_built, case):
    from octa_autosegmentation_amd import _native
    from octa_autosegmentation_amd.models import fused_ops
    x, dy, w, b, slope = nr.nchw_case(case, DEV)
    f32 = x.dtype == torch.float32
    xm, wm, bm = _leaf(x), _leaf(w), _leaf(b)
    y = fused_ops.instance_norm_leaky_relu(xm, wm, bm, slope, EPS)
    assert y.dtype == x.dtype and y.shape == x.shape
    y.backward(dy)
    got = _grads(dict(y=nr.bnc(y.detach(), "nchw"), dx=nr.bnc(xm.grad, "nchw")), wm, bm)
    B, C, n = x.shape[0], x.shape[1], x.shape[2] * x.shape[3]
    y2 = torch.empty_like(x)
    mean, rstd = torch.empty(B * C, dtype=torch.float32, device=DEV), torch.empty(B * C, dtype=torch.float32, device=DEV)
    _native.launch("octa_instnorm_lrelu_fwd", x.device, x, y2, w, b, mean, rstd, B, C, n, 0 if f32 else 1, float(slope), EPS)
    got["mean"], got["rstd"] = mean.view(B, C), rstd.view(B, C)
    r = nr.reference(nr.bnc(x, "nchw"), w, b, slope, EPS, dy=nr.bnc(dy, "nchw"))
    _report(f"nchw {case}", nr.ratios(r, nr.bounds(r, stat=nr.STAT_F32 if f32 else nr.STAT_BF16, f32=f32), got))
    assert torch.equal(y2, y.detach())          # no atomics on this path: the same call gives the same bits


# ---- (f) the zeroed ring of the context ----------------------------------------------------------------------------------------------

def test_zeroed_ring_laps_and_growth(hip_lib_built):
    """A slot of B = 4, C = 512 is 32 KB: one lap of the 4 MB ring is 128 calls, and 200 forward + backward iterations cross it three
    times; a head pass every 7th iteration shifts the position, and a B = 9 forward (73.7 KB x 64 > 4 MB) makes the ring grow. One
    split fixes the summation order, so every iteration must give the bits of the first."""
    from octa_autosegmentation_amd import _native
    gen = torch.Generator().manual_seed(4242)
    x = (torch.randn(4, 4, 4, 512, generator=gen) + 0.1).to(torch.bfloat16).to(DEV)
    dy = torch.randn(4, 4, 4, 512, generator=gen).to(torch.bfloat16).to(DEV)
    w, b = (torch.rand(512, generator=gen) + 0.5).to(DEV), (0.5 * torch.randn(512, generator=gen)).to(DEV)
    x9 = (torch.randn(9, 4, 4, 512, generator=gen) + 0.1).to(torch.bfloat16).to(DEV)
    hx, hdl, hw_, hb_, hhw, hhb, hslope = nr.head_case(8, 1, 1, 257, "affine", DEV)      # two splits: a + b into a zero, either order the same
    h = _native.new_ctx()
    try:
        with _native.use_ctx(h):
            first = _entry_both(x, dy, w, b, 0.01)
            r = nr.reference(nr.bnc(x, "nhwc"), w, b, 0.01, EPS, dy=nr.bnc(dy, "nhwc"))
            _report("ring, first iteration", nr.ratios(r, nr.bounds(r), first))
            head_first = None
            for it in range(1, 200):
                got = _entry_both(x, dy, w, b, 0.01)
                for k, v in first.items():
                    assert torch.equal(v, got[k]), (it, k)
                if it % 7 == 0:
                    hg = _entry_head(hx, hdl, hw_, hb_, hhw, hhb, hslope)
                    if head_first is None:
                        head_first = hg
                        rh = nr.reference(nr.bnc(hx, "nhwc"), hw_, hb_, hslope, EPS, head_w=hhw, head_b=hhb, dlogit=hdl)
                        _report("ring, head", nr.ratios(rh, nr.bounds(rh), hg))
                    for k in ("logits", "dx", "mean", "rstd"):
                        assert torch.equal(head_first[k], hg[k]), (it, k)
                if it == 100:
                    y9, m9, s9 = _entry_fwd(x9, w, b, 0.01)
                    r9 = nr.reference(nr.bnc(x9, "nhwc"), w, b, 0.01, EPS)
                    _report("ring, the forward that grows it", nr.ratios(r9, nr.bounds(r9), dict(y=nr.bnc(y9, "nhwc"), mean=m9, rstd=s9)))
            torch.cuda.synchronize()
    finally:
        torch.cuda.synchronize()
        _native.free_ctx(h)


# ---- (g) image groups (OCTA_NORM_CACHE_MB) -------------------------------------------------------------------------------------------

def test_image_group_path_in_a_fresh_process(hip_lib_built):
    """The budget is read once per process: one fresh child with OCTA_NORM_CACHE_MB=1 runs B = 3, 64 x 64, C = 64 (forward groups of
    2 + 1, backward image by image with cleared outputs and atomics) and compares with tests/_norm_ref.py itself."""
    env = dict(os.environ, OCTA_NORM_CACHE_MB="1")
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_norm_group_child.py")
    res = subprocess.run([sys.executable, script], env=env, timeout=180, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout[-4000:]
    assert "RATIO" in res.stdout


# ---- (h) refusals --------------------------------------------------------------------------------------------------------------------

def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


@pytest.mark.parametrize("C", [12, 520])
def test_plain_family_refuses_channel_counts(hip_lib_built, C):
    """C must be a multiple of 8 and at most 512; the check stands in front of every launch, so the outputs keep their NaN fill"""
    from octa_autosegmentation_amd import _native
    B, hw = 2, 16
    x = torch.zeros(B, 4, 4, C, dtype=torch.bfloat16, device=DEV)
    w = torch.ones(C, device=DEV)
    y, f = _nan(x.shape, torch.bfloat16), [_nan((B * C,), torch.float32) for _ in range(4)]
    dwb = _nan((2 * C,), torch.float32)
    calls = (
        ("octa_instnorm_lrelu_nhwc_fwd", (x, y, w, w, f[0], f[1], B, C, hw, 0.01, EPS, None, 0, None, 0)),
        ("octa_instnorm_lrelu_nhwc_bwd", (x, x, w, w, f[2], f[3], y, dwb[:C], dwb[C:], B, C, hw, 0.01)),
        ("octa_instnorm_nhwc_stats", (x, w, w, f[0], f[1], f[2], f[3], B, C, hw, EPS)),
        ("octa_scale_shift_lrelu_nhwc", (x, y, f[2], f[3], B, C, hw, 0.01)),
    )
    for name, args in calls:
        with pytest.raises(_native.OctaHipError):
            _native.launch(name, x.device, *args)
    torch.cuda.synchronize()
    for t in [y, dwb] + f:
        assert torch.isnan(t).all()


@pytest.mark.parametrize("C", [24, 512])
def test_head_refuses_channel_counts(hip_lib_built, C):
    """the fused head closes its dot product with lane exchanges: C / 8 must be a power of two, C <= 256"""
    from octa_autosegmentation_amd import _native
    B, hw = 2, 16
    x = torch.zeros(B, 4, 4, C, dtype=torch.bfloat16, device=DEV)
    dl = torch.zeros(B, 4, 4, 1, dtype=torch.bfloat16, device=DEV)
    w = torch.ones(C, device=DEV)
    hb = torch.ones(1, device=DEV)
    lg, dx = _nan(dl.shape, torch.bfloat16), _nan(x.shape, torch.bfloat16)
    mean, rstd = _nan((B * C,), torch.float32), _nan((B * C,), torch.float32)
    dgb, dhw, dhb = _nan((2 * C,), torch.float32), _nan((C,), torch.float32), _nan((1,), torch.float32)
    with pytest.raises(_native.OctaHipError):
        _native.launch("octa_instnorm_lrelu_head1_nhwc_fwd", x.device, x, w, w, w, hb, mean, rstd, lg, B, C, hw, 0.01, EPS, None, 0)
    with pytest.raises(_native.OctaHipError):
        _native.launch("octa_instnorm_lrelu_head1_nhwc_bwd", x.device, x, dl, w, w, w, mean, rstd, dx, dgb[:C], dgb[C:], dhw, dhb, B, C, hw, 0.01)
    torch.cuda.synchronize()
    for t in (lg, dx, mean, rstd, dgb, dhw, dhb):
        assert torch.isnan(t).all()
