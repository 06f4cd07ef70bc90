"""GPU: every bf16 MFMA convolution kernel of csrc/conv.hip against the float64 reference of tests/_conv_ref.py (proved on the CPU by
tests/test_conv_ref.py): exact cases bit for bit, real-valued cases inside the derived bound on every element. Direct calls of the entry
points (mfma_conv._conv3x3_fwd / _conv3x3_wgrad, the octa_conv3x3_nhwc_wgrad struct for the tap-major output, _native.launch for the others)
with every buffer a kernel writes -- outputs, the split output, statistics, weight gradients -- between sentinels; the reference is computed
in float64 on the device from the operands the kernel receives. Weight gradients that fold with atomics or slices, and statistics, run twice:
both runs meet the bound and the exact variant gives identical bits. Then the refusals of the host code (full-size buffers, nothing
written), the four parity classes of the scatter form in one output, and exact cases through autograd.

Each case prints a RATIO line (error / bound; 0 for an exact case) before it asserts. A GPU error ends the session (pytest.exit): nothing
more is started on a device that has faulted.

MEASURED on the MI355X (256 compute units) at r = _conv_ref.R_MFMA = 16 (one rounding per product); it did not have to be raised. Every exact
case has ratio 0 (forward outputs, statistics, the untouched parity classes of the scatter, every weight gradient); both runs of a repeated
case are bit-identical. Largest error / bound of the real-valued cases per family (the CPU emulation of tests/test_conv_ref.py in brackets):
    fwd      0.987  (0.987)   mask_centre, BN 64: the half bf16 ulp, which a value just above a power of two uses in full
    fwd_pad  0.971  (0.971)   s2t  0.986  (0.986)   fwd4  0.950  (0.950)
    wgrad    0.031  (0.039)   without normalise-on-load; 0.907 (0.907) with it (f64x32_norm: one input element whose bf16 rounding sits within
                              the fp32 error of a tie -- the allowance E of _conv_ref.normalise(), used almost in full, by kernel and emulation alike)
    wgrad_pad 0.023 (0.024)   wgrad4 0.046 (0.046)
The fp32 outputs stay below 0.05 of D * 2^-24 * S: one rounding per product (r = 16) is far more than the matrix cores apply, and r = 32 would
only halve these figures; the bf16 outputs are governed by the half ulp whatever r is.
"""
import ctypes

import pytest
import torch

import _conv_ref as cr
from _guarded import DEV, Guarded

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def _sync():
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:          # a faulted device: start nothing more on it
        pytest.exit(f"GPU error, session ended: {e}", returncode=3)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dev(ops):
    return {k: (v.to(DEV) if v is not None else None) for k, v in ops.items()}


def _norm(o):
    return (o.get("sc1"), o.get("sh1"), o.get("sc2"), o.get("sh2"))


def _wgrad_args(p, o, dw, **over):
    from octa_autosegmentation_amd import _native
    ad = _native.addr
    f = dict(struct_size=ctypes.sizeof(_native.Conv3x3WgradArgs), N=p.N, H=p.H, W=p.W, Cin=p.Cin, Cout=p.Cout, stride=p.stride, tap_mask=p.mask,
             C1=p.C1 or p.Cin, out_mode=p.mode, slope=float(p.slope), d_x=ad(o["x"]), d_x2=ad(o.get("x2")), d_dy=ad(o["dy"]), d_dw=ad(dw),
             d_scale1=ad(o.get("sc1")), d_shift1=ad(o.get("sh1")), d_scale2=ad(o.get("sc2")), d_shift2=ad(o.get("sh2")))
    f.update(over)
    return _native.Conv3x3WgradArgs(**f)


def _call(c, o):
    """One direct call of the entry point of case c on device operands o -> (got as _conv_ref.check takes it, [Guarded])"""
    from octa_autosegmentation_amd import _native
    from octa_autosegmentation_amd.models import mfma_conv
    p = c.p
    dev = o["x"].device
    Ho, Wo = cr.out_extent(p)
    if c.fam in cr.FORWARD:
        wt = mfma_conv.slice_major(o["w"])
        osc = p.scatter[0] if p.scatter else 1
        y = Guarded((p.N, Ho * osc, Wo * osc, p.CY1 or p.Cout), BF)
        y2 = Guarded((p.N, Ho, Wo, p.Cout - p.CY1), BF) if p.CY1 else None
        part = slots = None
        if p.stats == "tile":
            tiles = int(_native.lib().octa_conv_stat_tiles(Ho, Wo))
            assert tiles == ((Ho + 7) // 8) * ((Wo + 31) // 32)
            part = Guarded((p.N, tiles, p.Cout, 2), F32)             # every tile is written: no element may keep the sentinel
        elif p.stats is not None:
            slots = Guarded((p.stats, p.N, p.Cout, 2), F64)
            slots.t.zero_()                                          # the kernel accumulates into the slots
        guards = [g for g in (y, y2, part, slots) if g is not None]
        if c.fam == "fwd":
            mfma_conv._conv3x3_fwd(o["x"], wt, y.t, x2=o.get("x2"), y2=y2.t if y2 else None, stride=p.stride, in_dilation=p.dil, tap_mask=p.mask,
                                   scatter=p.scatter or (1, 0, 0), norm=_norm(o), slope=p.slope, stat_partials=part.t if part else None,
                                   stat_slots=slots.t if slots else None, residual=o.get("res"))
        elif c.fam == "fwd_pad":
            _native.launch("octa_conv3x3_nhwc_fwd_pad", dev, o["x"], wt, y.t, p.N, p.H, p.W, p.Cin, p.Cout, p.pad, p.reflect,
                           slots.t if slots else None, p.stats if slots else 0)
        elif c.fam == "s2t":
            _native.launch("octa_conv3x3_s2t_nhwc", dev, o["x"], wt, y.t, p.N, p.H, p.W, p.Cin, p.Cout, p.mask, o.get("res"))
        else:
            _native.launch("octa_conv4x4_nhwc_fwd", dev, o["x"], wt, y.t, p.N, p.H, p.W, p.Cin, p.Cout, p.pad)
        st = part.t if part else (slots.t if slots else None)
        return dict(y=y.t, y2=y2.t if y2 else None, stats=st), guards
    dw = Guarded((p.Cout, p.Cin, 3, 3) if p.mode else (p.K * p.K, p.Cout, p.Cin), F32)
    if p.mode == cr.PARAM_ADD:
        dw.t.copy_(o["base"])
    if c.fam == "wgrad" and p.mode:
        assert mfma_conv._conv3x3_wgrad(o["x"], o["dy"], o.get("x2"), into=dw.t, accumulate=p.mode == cr.PARAM_ADD, stride=p.stride, tap_mask=p.mask,
                                        norm=_norm(o), slope=p.slope) is None
    elif c.fam == "wgrad":             # the tap-major output into a guarded buffer: the struct as mfma_conv._conv3x3_wgrad fills it
        _native.launch("octa_conv3x3_nhwc_wgrad", dev, ctypes.byref(_wgrad_args(p, o, dw.t)))
    elif c.fam == "wgrad_pad":
        _native.launch("octa_conv3x3_nhwc_wgrad_pad", dev, o["x"], o["dy"], dw.t, p.N, p.H, p.W, p.Cin, p.Cout, p.pad, p.reflect, p.mode)
    else:
        _native.launch("octa_conv4x4_nhwc_wgrad", dev, o["x"], o["dy"], dw.t, p.N, p.H, p.W, p.Cin, p.Cout)
    return dict(dw=dw.t), [dw]


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _run_case(fam, name):
    variants = [v for f, n, v in cr.ALL if (f, n) == (fam, name)]
    for var in variants:
        c = cr.case(fam, name, var, _cus())           # asserts the instantiation and the fold path for THIS device's compute units
        o = _dev(c.ops)
        r = cr.ref_of(c, o)                           # float64, on the device, from the operands the kernel gets
        twice = c.p.stats is not None or (c.fam not in cr.FORWARD and c.d.fold in ("atomics", "slices"))
        runs = []
        for _ in range(2 if twice else 1):
            got, guards = _call(c, o)
            _sync()
            rat = cr.check(c, r, got)
            what = f"{c.d.inst}" + (f" fold={c.d.fold} per_block={c.d.per_block}" if fam not in cr.FORWARD else "")
            print("RATIO", f"{fam}/{name}/{var}", " ".join(f"{fam}.{k}={v:.4g}" for k, v in rat.items()), f"D={c.D}", what)
            assert all(gd.intact() for gd in guards), f"{fam}/{name}/{var}: a sentinel around an output was overwritten"
            if var == "exact":
                assert all(v == 0.0 for v in rat.values()), f"{fam}/{name}: not the one legal result, bit for bit ({rat}; {what})"
            else:
                assert all(v <= 1.0 for v in rat.values()), f"{fam}/{name}: error / bound above 1 ({rat}, D = {c.D}; {what})"
            runs.append(got)
        if twice and var == "exact":
            for k in runs[0]:
                if runs[0][k] is not None:
                    assert torch.equal(_bits(runs[0][k]), _bits(runs[1][k])), f"{fam}/{name}: two runs differ in {k}"


@pytest.mark.parametrize("name", list(cr.FAMILIES["fwd"]))
def test_fwd(hip_lib_built, name):
    _run_case("fwd", name)


@pytest.mark.parametrize("name", list(cr.FAMILIES["fwd_pad"]))
def test_fwd_pad(hip_lib_built, name):
    _run_case("fwd_pad", name)


@pytest.mark.parametrize("name", list(cr.FAMILIES["s2t"]))
def test_s2t(hip_lib_built, name):
    _run_case("s2t", name)


@pytest.mark.parametrize("name", list(cr.FAMILIES["fwd4"]))
def test_fwd4(hip_lib_built, name):
    _run_case("fwd4", name)


@pytest.mark.parametrize("name", list(cr.FAMILIES["wgrad"]))
def test_wgrad(hip_lib_built, name):
    _run_case("wgrad", name)


@pytest.mark.parametrize("name", list(cr.FAMILIES["wgrad_pad"]))
def test_wgrad_pad(hip_lib_built, name):
    _run_case("wgrad_pad", name)


@pytest.mark.parametrize("name", list(cr.FAMILIES["wgrad4"]))
def test_wgrad4(hip_lib_built, name):
    _run_case("wgrad4", name)


@pytest.mark.parametrize("bn", [32, 64])
def test_scatter_the_four_parity_classes_fill_one_output(hip_lib_built, bn):
    """out_scale = 2: one launch per (off_y, off_x) into ONE sentinel-filled image twice the size. After every launch the classes written so
    far hold the result and the others still hold the sentinel: a launch writes its own quarter of the pixels and nothing else."""
    from octa_autosegmentation_amd.models import mfma_conv
    c = cr.case("fwd", f"bn{bn}_scatter_00", "exact", _cus())
    o = _dev(c.ops)
    want = cr.once(cr.ref_of(c, o).acc)
    N, Ho, Wo, C = want.shape
    y = Guarded((N, 2 * Ho, 2 * Wo, C), BF)
    done = []
    for a, b in ((1, 0), (0, 1), (1, 1), (0, 0)):
        mfma_conv._conv3x3_fwd(o["x"], mfma_conv.slice_major(o["w"]), y.t, tap_mask=c.p.mask, scatter=(2, a, b))
        _sync()
        done.append((a, b))
        for aa in (0, 1):
            for bb in (0, 1):
                cls = y.t[:, aa::2, bb::2]
                if (aa, bb) in done:
                    assert torch.equal(cls, want), (done, aa, bb)
                else:
                    assert bool((_bits(cls) == cr.SENT_BITS).all()), (done, aa, bb)
        assert y.intact()


# ---- the refusals -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(cr.REFUSALS))
def test_refusals(hip_lib_built, name):
    """Each call gets buffers of the full size it could need, so that a missing refusal is a wrong answer and not an out-of-bounds access;
    after the refused call nothing has been written."""
    from octa_autosegmentation_amd import _native
    p, x = cr.REFUSALS[name]
    gen = torch.Generator().manual_seed(11)
    C1 = p.C1 or p.Cin
    big = p.N * (2 * p.H + 8) * (2 * p.W + 8)                      # pixels: more than any output extent of the call
    cpad = (max(p.Cin, p.Cout) + 63) // 64 * 64
    o = _dev(dict(x=cr._quarters((p.N, p.H, p.W, max(C1, 32)), 3, gen).to(BF), x2=cr._quarters((p.N, p.H, p.W, cpad), 3, gen).to(BF),
                  w=torch.ones((16, cpad, cpad), dtype=BF), res=cr._quarters((big, cpad), 4, gen).to(BF), dy=cr._quarters((big, cpad), 3, gen).to(BF),
                  sc=torch.ones((p.N, cpad)), sh=torch.zeros((p.N, cpad))))
    y, y2, dw = Guarded((big, cpad), BF), Guarded((big, cpad), BF), Guarded((16, cpad, cpad), F32)
    part, slots = Guarded((big, cpad, 2), F32), Guarded((1025, p.N, cpad, 2), F64)
    ad, dev = _native.addr, o["x"].device
    nslot = x.get("nslot", p.stats if isinstance(p.stats, int) else 0)
    want_slots = isinstance(p.stats, int) or "nslot" in x
    want_part = p.stats == "tile" or x.get("both_stats", False)
    res = None if not p.res else (y.t if x.get("res_alias") else o["res"])
    with pytest.raises(_native.OctaHipError):
        if p.kind == "fwd":
            osc, oy, ox = p.scatter or (1, 0, 0)
            a = _native.Conv3x3Args(
                struct_size=ctypes.sizeof(_native.Conv3x3Args) + (8 if x.get("struct_size_off") else 0), N=p.N, H=p.H, W=p.W, Cin=p.Cin, Cout=p.Cout,
                stride=p.stride, in_dilation=p.dil, tap_mask=p.mask, out_scale=osc, out_off_y=oy, out_off_x=ox, C1=C1, CY1=p.CY1 or p.Cout, nslot=nslot,
                slope=0.25, d_x=ad(o["x"]), d_x2=ad(o["x2"]) if p.C1 else None, d_w=ad(o["w"]), d_y=ad(y.t), d_y2=ad(y2.t) if p.CY1 else None,
                d_scale1=ad(o["sc"]) if p.norm else None, d_shift1=ad(o["sh"]) if p.norm else None, d_scale2=None, d_shift2=None,
                d_stat_partials=ad(part.t) if want_part else None, d_stat_slots=ad(slots.t) if want_slots else None, d_residual=ad(res))
            _native.launch("octa_conv3x3_nhwc_fwd", dev, ctypes.byref(a))
        elif p.kind == "fwd_pad":
            _native.launch("octa_conv3x3_nhwc_fwd_pad", dev, o["x"], o["w"], y.t, p.N, p.H, p.W, p.Cin, p.Cout, p.pad, p.reflect,
                           slots.t if want_slots else None, nslot)
        elif p.kind == "s2t":
            _native.launch("octa_conv3x3_s2t_nhwc", dev, o["x"], o["w"], y.t, p.N, p.H, p.W, p.Cin, p.Cout, p.mask, res)
        elif p.kind == "fwd4":
            _native.launch("octa_conv4x4_nhwc_fwd", dev, o["x"], o["w"], y.t, p.N, p.H, p.W, p.Cin, p.Cout, p.pad)
        elif p.kind == "wgrad":
            oo = dict(x=o["x"], x2=o["x2"] if p.C1 else None, dy=o["dy"], sc1=o["sc"] if p.norm else None, sh1=o["sh"] if p.norm else None)
            over = dict(struct_size=ctypes.sizeof(_native.Conv3x3WgradArgs) + 8) if x.get("struct_size_off") else {}
            _native.launch("octa_conv3x3_nhwc_wgrad", dev, ctypes.byref(_wgrad_args(p, oo, dw.t, **over)))
        elif p.kind == "wgrad_pad":
            _native.launch("octa_conv3x3_nhwc_wgrad_pad", dev, o["x"], o["dy"], dw.t, p.N, p.H, p.W, p.Cin, p.Cout, p.pad, p.reflect, p.mode)
        else:
            _native.launch("octa_conv4x4_nhwc_wgrad", dev, o["x"], o["dy"], dw.t, p.N, p.H, p.W, p.Cin, p.Cout)
    _sync()
    for buf in (y, y2, dw, part, slots):
        assert buf.untouched(), f"{name}: a refused call wrote"


# ---- exact cases through autograd --------------------------------------------------------------------------------------------------------------
# forward and all gradients in float64 on the CPU, rounded once; shapes of a few pixels; USE_DIRECT_WGRAD at its default, outside a backward scope

def _weight(gen, *shape):
    return cr._quarters(shape, 2, gen, zero_half=True).to(DEV).requires_grad_(True)


def _act(gen, *shape):
    return cr._quarters(shape, 3, gen).to(BF).to(DEV)


def _nchw64(t):
    return t.detach().double().cpu().permute(0, 3, 1, 2)


def _backward_twice(y, dy, leaves):
    """-> the gradients of `leaves`; the backward runs twice and has to give identical bits"""
    runs = []
    for _ in range(2):
        for t in leaves:
            t.grad = None
        y.backward(dy, retain_graph=True)
        _sync()
        runs.append([t.grad.clone() for t in leaves])
    for g0, g1 in zip(*runs):
        assert torch.equal(_bits(g0), _bits(g1)), "two backward passes differ"
    return runs[0]


def _same(got, want64_nchw, what):
    """got NHWC (bf16: the float64 result rounded once) or a weight gradient (fp32: the float64 result itself)"""
    if got.dtype == BF:
        assert torch.equal(got.detach().cpu(), cr.once(want64_nchw.permute(0, 2, 3, 1))), f"{what}: not the float64 result rounded once"
    else:
        assert got.dtype == F32 and torch.equal(got.detach().cpu(), want64_nchw.float()) and torch.equal(want64_nchw.float().double(), want64_nchw), \
            f"{what}: not the float64 result"


def _f64(fn, dy, *leaves):
    """float64 autograd on the CPU: fn(*leaves) -> y; -> (y, gradients)"""
    ls = [t.clone().requires_grad_(True) for t in leaves]
    y = fn(*ls)
    y.backward(_nchw64(dy))
    return y.detach(), [t.grad for t in ls]


@pytest.mark.parametrize("stride,n,h,w,cin,cout", [(1, 2, 3, 5, 32, 64), (1, 1, 9, 33, 64, 32), (2, 2, 4, 6, 32, 32), (2, 1, 10, 66, 32, 64)])
def test_conv3x3_exact_through_autograd(hip_lib_built, stride, n, h, w, cin, cout):
    from octa_autosegmentation_amd.models import mfma_conv
    assert mfma_conv.USE_DIRECT_WGRAD
    gen = torch.Generator().manual_seed(100 * h + stride)
    wt, x = _weight(gen, cout, cin, 3, 3), _act(gen, n, h, w, cin).requires_grad_(True)
    y = mfma_conv.conv3x3(x, wt, stride)
    dy = _act(gen, *y.shape)
    dx, dw = _backward_twice(y, dy, [x, wt])
    y_ref, (dx_ref, dw_ref) = _f64(lambda a, b: torch.nn.functional.conv2d(a, b, stride=stride, padding=1), dy, _nchw64(x), wt.detach().double().cpu())
    _same(y, y_ref, "y")
    _same(dx, dx_ref, "dx")
    _same(dw, dw_ref, "dw")


@pytest.mark.parametrize("n,h,w,c1,c2,cout", [(2, 3, 5, 32, 32, 32), (1, 5, 4, 64, 32, 64), (1, 2, 33, 32, 64, 96)])
def test_conv3x3_cat_exact_through_autograd(hip_lib_built, n, h, w, c1, c2, cout):
    from octa_autosegmentation_amd.models import mfma_conv
    gen = torch.Generator().manual_seed(200 + c1 + h)
    wt = _weight(gen, cout, c1 + c2, 3, 3)
    x1, x2 = _act(gen, n, h, w, c1).requires_grad_(True), _act(gen, n, h, w, c2).requires_grad_(True)
    y = mfma_conv.conv3x3_cat(x1, x2, wt)
    dy = _act(gen, *y.shape)
    d1, d2, dw = _backward_twice(y, dy, [x1, x2, wt])
    y_ref, (r1, r2, rw) = _f64(lambda a, b, k: torch.nn.functional.conv2d(torch.cat((a, b), 1), k, padding=1), dy, _nchw64(x1), _nchw64(x2), wt.detach().double().cpu())
    _same(y, y_ref, "y")
    _same(d1, r1, "dx1")
    _same(d2, r2, "dx2")
    _same(dw, rw, "dw")


@pytest.mark.parametrize("n,h,w,cin,cout", [(2, 2, 2, 32, 32), (1, 3, 5, 32, 64), (1, 9, 33, 64, 64)])
def test_conv3x3_reflect_exact_through_autograd(hip_lib_built, n, h, w, cin, cout):
    """the data gradient is the full (pad 2) convolution of dy, stored as bf16, folded back by the reflection's adjoint and stored as bf16
    again: two roundings where mirrored pixels meet, and the reference applies the same two"""
    from octa_autosegmentation_amd.models import mfma_conv
    F = torch.nn.functional
    gen = torch.Generator().manual_seed(300 + h)
    wt, x = _weight(gen, cout, cin, 3, 3), _act(gen, n, h, w, cin).requires_grad_(True)
    y = mfma_conv.conv3x3_reflect(x, wt)
    dy = _act(gen, *y.shape)
    dx, dw = _backward_twice(y, dy, [x, wt])
    xp = F.pad(_nchw64(x), (1, 1, 1, 1), mode="reflect")
    y_ref, (dxp_ref, dw_ref) = _f64(lambda a, b: F.conv2d(a, b), dy, xp, wt.detach().double().cpu())
    dxp = cr.once(dxp_ref).double()                                   # first rounding: the padded gradient as the kernel stores it
    z = torch.zeros((n, cin, h, w), dtype=torch.float64, requires_grad=True)
    F.pad(z, (1, 1, 1, 1), mode="reflect").backward(dxp)              # the adjoint of the reflection: at most four bf16 numbers per pixel, exact in fp32
    _same(y, y_ref, "y")
    _same(dx, z.grad, "dx")
    _same(dw, dw_ref, "dw")


@pytest.mark.parametrize("n,h,w,cin,cout", [(2, 1, 1, 32, 32), (1, 3, 5, 64, 32), (1, 9, 33, 32, 96)])
def test_conv_transpose_2x2_exact_through_autograd(hip_lib_built, n, h, w, cin, cout):
    from octa_autosegmentation_amd.models import mfma_conv
    gen = torch.Generator().manual_seed(400 + h)
    wt, x = _weight(gen, cin, cout, 2, 2), _act(gen, n, h, w, cin).requires_grad_(True)
    y = mfma_conv.conv_transpose_kxk_nhwc(x, wt, 2)
    assert y.shape == (n, 2 * h, 2 * w, cout)
    dy = _act(gen, *y.shape)
    dx, dw = _backward_twice(y, dy, [x, wt])
    y_ref, (dx_ref, dw_ref) = _f64(lambda a, b: torch.nn.functional.conv_transpose2d(a, b, stride=2), dy, _nchw64(x), wt.detach().double().cpu())
    _same(y, y_ref, "y")
    _same(dx, dx_ref, "dx")
    _same(dw, dw_ref, "dw")


@pytest.mark.parametrize("n,h,w,cin,cout", [(2, 2, 2, 32, 32), (1, 5, 6, 64, 64), (1, 9, 34, 32, 64)])
def test_conv4x4_exact_through_autograd(hip_lib_built, n, h, w, cin, cout):
    from octa_autosegmentation_amd.models import mfma_conv
    gen = torch.Generator().manual_seed(500 + h)
    wt, x = _weight(gen, cout, cin, 4, 4), _act(gen, n, h, w, cin).requires_grad_(True)
    y = mfma_conv.conv4x4(x, wt)
    dy = _act(gen, *y.shape)
    dx, dw = _backward_twice(y, dy, [x, wt])
    y_ref, (dx_ref, dw_ref) = _f64(lambda a, b: torch.nn.functional.conv2d(a, b, padding=1), dy, _nchw64(x), wt.detach().double().cpu())
    _same(y, y_ref, "y")
    _same(dx, dx_ref, "dx")
    _same(dw, dw_ref, "dw")


@pytest.mark.parametrize("stride,two,n,h,w,cout", [(1, False, 2, 3, 5, 32), (1, True, 1, 5, 4, 64), (2, False, 2, 4, 6, 64)])
def test_conv3x3_lazy_exact_through_autograd(hip_lib_built, stride, two, n, h, w, cout):
    """normalise-on-load through autograd: the tensors stand for lrelu(t scale + shift) in the graph, so their gradients are those of the
    normalised activations"""
    from octa_autosegmentation_amd.models import mfma_conv
    gen = torch.Generator().manual_seed(600 + h + stride)
    slope, c = 0.25, 32
    ts, lazies, xn = [], [], []
    for _ in range(2 if two else 1):
        t = _act(gen, n, h, w, c).requires_grad_(True)
        sc = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (n, c), generator=gen)].to(DEV)
        sh = cr._quarters((n, c), 2, gen).to(DEV)
        q, _, exact = cr.normalise(t.detach(), sc, sh, slope)
        assert exact
        ts.append(t)
        lazies.append((t, sc.reshape(-1), sh.reshape(-1)))
        xn.append(q.cpu().permute(0, 3, 1, 2))
    wt = _weight(gen, cout, c * len(ts), 3, 3)
    y = mfma_conv.conv3x3_lazy(lazies[0], wt, stride, lazies[1] if two else None, slope)
    dy = _act(gen, *y.shape)
    grads = _backward_twice(y, dy, ts + [wt])
    y_ref, refs = _f64(lambda *a: torch.nn.functional.conv2d(torch.cat(a[:-1], 1), a[-1], stride=stride, padding=1), dy, *xn, wt.detach().double().cpu())
    _same(y, y_ref, "y")
    for i, (g, r) in enumerate(zip(grads, refs)):
        _same(g, r, f"gradient {i}")
