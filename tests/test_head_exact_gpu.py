"""GPU: the kernels of csrc/head.hip against the float64 reference of tests/_head_ref.py (proved on the CPU by tests/test_head_ref.py): exact
cases bit for bit, real-valued cases inside the derived bound on every element. Direct calls of octa_headn_nhwc_fwd / octa_headn_nhwc_bwd
through _native.launch with every buffer a kernel writes (y, dx, dw, db) between sentinels, y and dy at the element offset the case names;
the reference is computed in float64 on the device from the operands the kernel receives. Every case runs twice and both runs have to give
identical bits. Then a small call behind the largest one (stale partials in the context's workspace), the autograd binding on an fp32
master weight, and the refusals of the host code.

Each case prints a RATIO line (error / bound; 0 for an exact case) before it asserts. A GPU error ends the session (pytest.exit): nothing
more is started on a device that has faulted.

MEASURED on the MI355X (256 compute units), on the kernels as the commit that adds this file found them (csrc/head.hip is unchanged). Every
exact case has ratio 0 for y, dx, dw and db, the loop cases among them; both runs of every case are bit-identical. Largest error / bound of
the real-valued cases (the CPU emulation of tests/test_head_ref.py in brackets):
    y  0.994 (0.994)      dx  0.996 (0.996)      dw  0.0138 (0.0219)      db  0.0019 (0.0019)
y and dx are governed by the half bf16 ulp, which a value just above a power of two uses in full; dw and db stay far below D * 2^-24 * S:
one rounding per product is more than the matrix cores apply.
"""
from types import SimpleNamespace

import pytest
import torch

import _head_ref as hr
from _guarded import DEV, Guarded

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32


def _sync():
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:          # a faulted device: start nothing more on it
        pytest.exit(f"GPU error, session ended: {e}", returncode=3)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dev(ops):
    return {k: (v.to(DEV) if v is not None else None) for k, v in ops.items()}


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _call(c, o):
    """One forward and one backward call of case c on device operands o -> (got as _head_ref.check takes it, name -> Guarded)"""
    from octa_autosegmentation_amd import _native
    p, N, hw = c.p, c.N, c.hw
    y = Guarded((N, p.Cout, hw), BF, offset=p.off)
    dy = Guarded((N, p.Cout, hw), BF, offset=p.off)              # the gradient the kernel reads, at the same offset
    dy.t.copy_(o["dy"])
    dx, dw, db = Guarded((N, hw, p.Cin), BF), Guarded((p.Cout, p.Cin), F32), Guarded((p.Cout,), F32)
    assert y.t.data_ptr() % 16 == (2 * p.off) % 16 and dy.t.data_ptr() % 16 == (2 * p.off) % 16 and dx.t.data_ptr() % 16 == 0
    _native.launch("octa_headn_nhwc_fwd", o["x"].device, o["x"], o["w"], o["b"], N, hw, p.Cin, p.Cout, y.t)
    _native.launch("octa_headn_nhwc_bwd", o["x"].device, o["x"], dy.t, o["w"], N, hw, p.Cin, p.Cout, dx.t, dw.t, db.t if p.db else None)
    _sync()
    got = dict(y=y.t, dx=dx.t, dw=dw.t)
    if p.db:
        got["db"] = db.t
    return got, dict(y=y, dy=dy, dx=dx, dw=dw, db=db)


def _run_case(name, var, worst=None):
    c = hr.case(name, var, _cus())                # asserts the loops and the tile counts for THIS device's compute units
    o = _dev(c.ops)
    r = hr.ref_of(c, o)                           # float64, on the device, from the operands the kernel gets
    runs = []
    for _ in range(2):
        got, gd = _call(c, o)
        rat = hr.check(c, r, got)
        print("RATIO", f"{name}/{var}", " ".join(f"{k}={v:.4g}" for k, v in rat.items()), f"D={c.D}", c.d.fwd, c.d.bwd,
              f"tiles={c.d.ntiles} fwd_wgs={c.d.fwd_wgs} nparts={c.d.nparts}")
        assert all(g.intact() for g in gd.values()), f"{name}/{var}: a sentinel around a buffer was overwritten"
        assert torch.equal(gd["dy"].t, o["dy"]), f"{name}/{var}: the kernel's input changed"
        for k in got:
            assert gd[k].unwritten() == 0, f"{name}/{var}: {gd[k].unwritten()} elements of {k} were never stored"
        if not c.p.db:
            assert gd["db"].untouched(), f"{name}/{var}: a null d_db, and the buffer was written"
        if var == "exact":
            assert all(v == 0.0 for v in rat.values()), f"{name}: not the one legal result, bit for bit ({rat})"
        else:
            assert all(v <= 1.0 for v in rat.values()), f"{name}: error / bound above 1 ({rat}, D = {c.D})"
            if worst is not None:
                for k, v in rat.items():
                    worst[k] = max(worst.get(k, 0.0), v)
        runs.append(got)
    for k in runs[0]:
        assert torch.equal(_bits(runs[0][k]), _bits(runs[1][k])), f"{name}/{var}: two runs differ in {k}"
    return runs[0]


WORST = {}


@pytest.mark.parametrize("name", hr.SMALL)
def test_case(hip_lib_built, name):
    for var in [v for n, v in hr.ALL if n == name]:
        _run_case(name, var, WORST)
    print("WORST so far", {k: float(f"{v:.4g}") for k, v in WORST.items()})


@pytest.mark.parametrize("name", hr.LOOP)
def test_loop_case(hip_lib_built, name):
    _run_case(name, "exact")


def test_small_call_after_the_largest_sees_no_stale_partials(hip_lib_built):
    """the largest backward leaves 2 * CUs partials in the context's workspace; the smallest case (one tile, one partial) right behind it, in
    the same process and context, has to give its own reference"""
    big = max(hr.LOOP, key=lambda n: hr.case(n, "exact", _cus()).d.nparts * hr.case(n, "exact", _cus()).d.KP)
    small = min(hr.SMALL, key=lambda n: hr.case(n, "exact", _cus()).N * hr.case(n, "exact", _cus()).hw)
    assert hr.case(big, "exact", _cus()).d.nparts > hr.RED_SPLIT and hr.case(small, "exact", _cus()).d.nparts == 1
    _run_case(big, "exact")
    _run_case(small, "exact")
    _run_case("red_17", "exact")
    _run_case(small, "real")


def test_binding_rounds_an_fp32_master_weight_inside_the_kernel(hip_lib_built):
    """mfma_conv.conv1x1_bias_nhwc with an fp32 master weight that is no bf16 number: the result is the kernel's on weight.float(), the
    gradients are the entry points' bit for bit (cast to the parameter's dtype), and both meet the reference's bounds"""
    from octa_autosegmentation_amd import _native
    from octa_autosegmentation_amd.models import mfma_conv
    n, h, w_, cin, cout = 2, 5, 7, 32, 5
    gen = torch.Generator().manual_seed(77)
    x = torch.randn((n, h, w_, cin), generator=gen).to(BF).to(DEV)
    dy = torch.randn((n, cout, h, w_), generator=gen).to(BF).to(DEV)
    for wdtype in (F32, BF):
        wm = (torch.randn((cout, cin, 1, 1), generator=gen) / cin ** 0.5).to(DEV).to(wdtype)
        bm = torch.randn((cout,), generator=gen).to(DEV).to(wdtype)
        if wdtype == F32:
            assert not torch.equal(wm.to(BF).float(), wm)
        wp, bp, xp = wm.clone().requires_grad_(True), bm.clone().requires_grad_(True), x.clone().requires_grad_(True)
        y = mfma_conv.conv1x1_bias_nhwc(xp, wp, bp)
        assert y.shape == (n, cout, h, w_) and y.is_contiguous() and y.dtype == BF
        y.backward(dy)
        _sync()
        wv, bv = wm.reshape(cout, cin).float().contiguous(), bm.float().contiguous()
        yk, dxk = Guarded((n, cout, h * w_), BF), Guarded((n, h * w_, cin), BF)
        dwk, dbk = Guarded((cout, cin), F32), Guarded((cout,), F32)
        _native.launch("octa_headn_nhwc_fwd", x.device, x, wv, bv, n, h * w_, cin, cout, yk.t)
        _native.launch("octa_headn_nhwc_bwd", x.device, x, dy, wv, n, h * w_, cin, cout, dxk.t, dwk.t, dbk.t)
        _sync()
        assert torch.equal(_bits(y.detach().view(n, cout, -1)), _bits(yk.t)) and torch.equal(_bits(xp.grad.view(n, -1, cin)), _bits(dxk.t))
        assert wp.grad.dtype == wdtype and wp.grad.shape == wm.shape and bp.grad.dtype == wdtype
        assert torch.equal(_bits(wp.grad.view(cout, cin)), _bits(dwk.t.to(wdtype))) and torch.equal(_bits(bp.grad), _bits(dbk.t.to(wdtype)))
        # and the entry points' results are the reference's for these operands, rounding of the weight included
        o = dict(x=x.view(n, h * w_, cin), w=wv, b=bv, dy=dy.view(n, cout, h * w_))
        cc = SimpleNamespace(var="real", D=hr.chain(cin, hr.dispatch(n, h * w_, cin, cout, _cus())), name="binding")
        rat = hr.check(cc, hr.reference(o), dict(y=yk.t, dx=dxk.t, dw=dwk.t, db=dbk.t))
        print("RATIO binding", wdtype, rat)
        assert all(v <= 1.0 for v in rat.values()), rat


def _refusal_buffers():
    gen = torch.Generator().manual_seed(5)
    o = _dev(dict(x=torch.randn((1, 16, 128), generator=gen).to(BF), dy=torch.randn((1, 65, 16), generator=gen).to(BF),
                  w=torch.randn((65, 128), generator=gen), b=torch.randn((65,), generator=gen)))
    return o, dict(y=Guarded((1, 65, 16), BF), dx=Guarded((1, 16, 128), BF), dw=Guarded((65, 128), F32), db=Guarded((65,), F32))


@pytest.mark.parametrize("name", list(hr.REFUSALS))
def test_refused_shapes(hip_lib_built, name):
    """Buffers of the full size a 16-pixel call could need, so that a missing refusal of a small shape is a wrong answer and no out-of-bounds
    access; the 2^30 cases are refused on their arguments (a missing refusal there would run past every buffer: the refusal is read from
    headn_check and mirrored by _head_ref.refusal before the call is made)."""
    from octa_autosegmentation_amd import _native
    N, hw, Cin, Cout = hr.REFUSALS[name]
    assert hr.refusal(N, hw, Cin, Cout)
    o, g = _refusal_buffers()
    with pytest.raises(_native.OctaHipError):
        _native.launch("octa_headn_nhwc_fwd", o["x"].device, o["x"], o["w"], o["b"], N, hw, Cin, Cout, g["y"].t)
    with pytest.raises(_native.OctaHipError):
        _native.launch("octa_headn_nhwc_bwd", o["x"].device, o["x"], o["dy"], o["w"], N, hw, Cin, Cout, g["dx"].t, g["dw"].t, g["db"].t)
    _sync()
    assert all(b.untouched() for b in g.values()), f"{name}: a refused call wrote"


@pytest.mark.parametrize("null", ["x", "w", "y", "dy", "dx", "dw"])
def test_refused_null_pointers(hip_lib_built, null):
    from octa_autosegmentation_amd import _native
    o, g = _refusal_buffers()
    a = dict(x=o["x"], w=o["w"], b=o["b"], dy=o["dy"], y=g["y"].t, dx=g["dx"].t, dw=g["dw"].t, db=g["db"].t)
    a[null] = None
    if null in ("x", "w", "y"):
        with pytest.raises(_native.OctaHipError, match="null pointer"):
            _native.launch("octa_headn_nhwc_fwd", o["x"].device, a["x"], a["w"], a["b"], 1, 16, 32, 4, a["y"])
    if null != "y":
        with pytest.raises(_native.OctaHipError, match="null pointer"):
            _native.launch("octa_headn_nhwc_bwd", o["x"].device, a["x"], a["dy"], a["w"], 1, 16, 32, 4, a["dx"], a["dw"], a["db"])
    _sync()
    assert all(b.untouched() for b in g.values()), f"null {null}: a refused call wrote"
