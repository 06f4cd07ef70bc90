"""GPU: every fp32 MFMA convolution kernel of csrc/conv_f32.hip against the float64 reference of tests/_conv_f32_ref.py (proved on the CPU by
tests/test_conv_f32_ref.py): exact cases bit for bit, real-valued cases inside the derived bound on every element. Direct calls of the five
entry points through _native.launch with every buffer a kernel writes -- y, dx, dW, db and the workspace, at exactly the byte count the library
reports -- between sentinels; the reference is computed in float64 on the device from the operands the kernel receives. A scattered launch
must leave every element outside its parity class as it was. Weight and bias gradients run twice and give identical bits. Then the refusals of
the host code (full-size buffers, the documented message, nothing written), the four parity classes of the scatter form in one output, and
exact layers through the binding (conv_f32.forward, conv_f32.train_forward with autograd.grad), which pins _packed, dgrad_layout and both
caches.

Each case prints a RATIO line (error / bound; 0 for an exact case) before it asserts. A GPU error ends the session (pytest.exit): nothing more
is started on a device that has faulted.

MEASURED on the MI355X (256 compute units), r = 2 roundings per instruction; nothing had to be raised. Every exact case has ratio 0 (outputs,
the untouched parity classes of the scatter, weight and bias gradients); both runs of every gradient case are bit-identical. Largest error /
bound of the real-valued cases per kind -- to the printed digits the figures of the CPU emulation of tests/test_conv_f32_ref.py:
    fwd 0.337 (k1s1_scatter_10)   tr 0.454 (7_64_n3)   dgrad 0.276 (c32_odd_n3)   wgrad dw 0.119 (c32_ho1)   db 0.017 (t22_ho2_n3)
These are measurements of the kernels against the float64 reference (also in DESIGN.md); they are never used as a tolerance.
"""
import ctypes

import pytest
import torch

import _conv_f32_ref as cr
from _guarded import DEV, Guarded

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


def _sync():
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:          # a faulted device: start nothing more on it
        pytest.exit(f"GPU error, session ended: {e}", returncode=3)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dev(ops):
    return {k: v.to(DEV) for k, v in ops.items()}


def _workspace_bytes(N, Cin, H, W, Cout, K, s, pad, Ho, Wo):
    from octa_autosegmentation_amd import _native
    nbytes = ctypes.c_size_t(0)
    _native.call("octa_conv2d_f32_wgrad_workspace", N, Cin, H, W, Cout, K, s, pad, Ho, Wo, ctypes.byref(nbytes))
    return nbytes.value


def _call(c, o):
    """One direct call of the entry point of case c on device operands o -> (got as _conv_f32_ref.check takes it, [Guarded])"""
    from octa_autosegmentation_amd import _native
    p, dev = c.p, torch.device(DEV, torch.cuda.current_device())
    if c.fam == "wgrad":
        a, b = (o["dy"], o["x"]) if p.transposed else (o["x"], o["dy"])
        N, Cin, H, W, Cout, Ho, Wo = cr.wgrad_operands(p)
        assert a.shape == (N, Cin, H, W) and b.shape == (N, Cout, Ho, Wo)
        nbytes = _workspace_bytes(N, Cin, H, W, Cout, p.K, p.stride, p.pad, Ho, Wo)
        assert nbytes == c.d.bytes, f"{c.name}: the library asks for {nbytes} bytes of workspace, the mirror of plan_wgrad for {c.d.bytes}"
        ws, dw, db = Guarded((nbytes // 4,), F32), Guarded((Cout, Cin, p.K, p.K), F32), Guarded((Cout,), F32)
        _native.launch("octa_conv2d_f32_wgrad_nchw", dev, a, b, dw.t, db.t, ws.t, nbytes, N, Cin, H, W, Cout, p.K, p.stride, p.pad, Ho, Wo)
        return dict(dw=dw.t, db=db.t), [ws, dw, db]
    L0 = c.Ls[0]
    y = Guarded((L0.N, L0.Cout, L0.Hy, L0.Wy), F32)
    if c.fam == "fwd":
        osc, a, b = p.scatter or (1, 0, 0)
        _native.launch("octa_conv2d_f32_nchw", dev, o["x"], o["wbuf"].data_ptr() + 4 * p.w_off, o.get("bias"), y.t, p.N, p.Cin, p.H, p.W, p.Cout, p.cout_w,
                       p.K, p.stride, p.pad, p.Ho, p.Wo, osc, a, b)
    elif c.fam == "tr":
        _native.launch("octa_convtranspose2x2_f32_nchw", dev, o["x"], o["wp"], y.t, p.N, p.Cin, p.H, p.W, p.Cout)
    else:
        _native.launch("octa_conv2d_f32_dgrad_nchw", dev, o["dy"], o["wp"], y.t, p.N, p.Cin, p.H, p.W, p.Cout, p.K, p.stride, p.pad, p.Ho, p.Wo, int(p.transposed))
    return dict(y=y.t), [y]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run_case(fam, name):
    for var in [v for f, n, v in cr.ALL if (f, n) == (fam, name)]:
        c = cr.case(fam, name, var, _cus())           # asserts the instantiations for THIS device's compute units
        o = _dev(c.ops)
        r = cr.ref_of(c, o, _cus())                   # float64, on the device, from the operands the kernel gets
        if fam in ("tr", "dgrad"):
            o["wp"] = cr.packed_weights(c.p, o).contiguous()      # models/conv_f32._packed / dgrad_layout: the binding's packing
        runs = []
        for _ in range(2 if fam == "wgrad" else 1):
            got, guards = _call(c, o)
            _sync()
            rat = cr.check(c, r, got)
            what = " ".join(c.insts) + (f" nchunks={c.d.nchunks} rounds={c.d.rounds} D={c.d.D} D_bias={c.d.D_bias}" if fam == "wgrad" else f" D={[L.D for L in c.Ls]}")
            print("RATIO", f"{fam}/{name}/{var}", " ".join(f"{fam}.{k}={v:.4g}" for k, v in rat.items()), what)
            assert all(gd.intact() for gd in guards), f"{fam}/{name}/{var}: a sentinel around a written buffer was overwritten"
            if var == "exact":
                assert all(v == 0.0 for v in rat.values()), f"{fam}/{name}: not the one legal result, bit for bit ({rat}; {what})"
            else:
                assert all(v <= 1.0 for v in rat.values()), f"{fam}/{name}: error / bound above 1 ({rat}; {what})"
            runs.append(got)
        if len(runs) == 2:
            for k in runs[0]:
                assert torch.equal(_bits(runs[0][k]), _bits(runs[1][k])), f"{fam}/{name}/{var}: two runs differ in {k}"


@pytest.mark.parametrize("name", list(cr.FAMILIES["fwd"]))
def test_fwd(hip_lib_built, name):
    _run_case("fwd", name)


@pytest.mark.parametrize("name", list(cr.FAMILIES["tr"]))
def test_tr(hip_lib_built, name):
    _run_case("tr", name)


@pytest.mark.parametrize("name", list(cr.FAMILIES["dgrad"]))
def test_dgrad(hip_lib_built, name):
    _run_case("dgrad", name)


@pytest.mark.parametrize("name", list(cr.FAMILIES["wgrad"]))
def test_wgrad(hip_lib_built, name):
    _run_case("wgrad", name)


def test_scatter_the_four_parity_classes_fill_one_output_and_equal_the_one_launch_form(hip_lib_built):
    """osc = 2: one 1x1 launch per (ooy, oox) into ONE sentinel-filled image twice the size. After every launch the classes written so far hold
    the float64 result and the others still hold the sentinel; the finished image has the bits of octa_convtranspose2x2_f32_nchw on the same
    packed weights -- and both are the reference, not merely each other."""
    from octa_autosegmentation_amd import _native
    c = cr.case("fwd", "k1s1_scatter_00", "exact", _cus())
    p, o = c.p, _dev(c.ops)
    dev = torch.device(DEV, torch.cuda.current_device())
    pt = cr.params("tr", N=p.N, Cin=p.Cin, Cout=p.Cout, H=p.H, W=p.W)
    r = cr.assemble(o["x"], o["wbuf"], cr.launches(pt, _cus()))
    assert torch.equal(r.ref.float().double(), r.ref) and r.S.max().item() < 2.0 ** 20
    want = r.ref.float()
    y = Guarded(want.shape, F32)
    done = []
    for a, b in ((1, 0), (0, 1), (1, 1), (0, 0)):
        _native.launch("octa_conv2d_f32_nchw", dev, o["x"], o["wbuf"].data_ptr() + 4 * (2 * a + b) * p.Cout, None, y.t, p.N, p.Cin, p.H, p.W, p.Cout, 4 * p.Cout,
                       1, 1, 0, p.H, p.W, 2, a, b)
        _sync()
        done.append((a, b))
        for aa in (0, 1):
            for bb in (0, 1):
                cls = y.t[:, :, aa::2, bb::2]
                if (aa, bb) in done:
                    assert torch.equal(cls, want[:, :, aa::2, bb::2]), (done, aa, bb)
                else:
                    assert bool((_bits(cls) == cr.SENT_BITS).all()), (done, aa, bb)
        assert y.intact()
    one = Guarded(want.shape, F32)
    _native.launch("octa_convtranspose2x2_f32_nchw", dev, o["x"], o["wbuf"], one.t, p.N, p.Cin, p.H, p.W, p.Cout)
    _sync()
    assert one.intact() and torch.equal(_bits(one.t), _bits(want)) and torch.equal(_bits(one.t), _bits(y.t))


# ---- the refusals -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(cr.REFUSALS))
def test_refusals(hip_lib_built, name):
    """Each call gets buffers of the full size it could need, so that a missing refusal is a wrong answer and not an out-of-bounds access; it
    raises with the documented message, and after the refused call nothing has been written."""
    from octa_autosegmentation_amd import _native
    p = cr.REFUSALS[name]
    why = cr.refusal(p)
    assert why
    gen = torch.Generator().manual_seed(11)
    dev = torch.device(DEV, torch.cuda.current_device())
    ch = max(p.Cin, p.Cout, p.cout_w)
    big = p.N * ch * (2 * max(p.H, p.Ho) + 8) * (2 * max(p.W, p.Wo) + 8)          # elements: more than any tensor of the call
    x, dy = cr._quarters((big,), 3, gen).to(DEV), cr._quarters((big,), 3, gen).to(DEV)
    w = torch.ones((64 * ch * ch + 64,), dtype=F32, device=DEV)
    bias = torch.ones((ch,), dtype=F32, device=DEV)
    y, dw, db = Guarded((big,), F32), Guarded((64 * ch * ch,), F32), Guarded((ch,), F32)
    N, Cin, H, W, Cout, Ho, Wo = cr.wgrad_operands(p)
    nbytes = _workspace_bytes(N, Cin, H, W, Cout, p.K, p.stride, max(p.pad, 0), Ho, Wo) if p.kind == "wgrad" else 4
    ws = Guarded((nbytes // 4,), F32)
    with pytest.raises(_native.OctaHipError) as e:
        if p.kind == "fwd":
            osc, a, b = p.scatter or (1, 0, 0)
            _native.launch("octa_conv2d_f32_nchw", dev, x, w, bias, y.t, p.N, p.Cin, p.H, p.W, p.Cout, p.cout_w, p.K, p.stride, p.pad, p.Ho, p.Wo, osc, a, b)
        elif p.kind == "tr":
            _native.launch("octa_convtranspose2x2_f32_nchw", dev, x, w, y.t.data_ptr() + (4 if p.misalign else 0), p.N, p.Cin, p.H, p.W, p.Cout)
        elif p.kind == "dgrad":
            _native.launch("octa_conv2d_f32_dgrad_nchw", dev, dy, w, y.t, p.N, p.Cin, p.H, p.W, p.Cout, p.K, p.stride, p.pad, p.Ho, p.Wo, int(p.transposed))
        else:
            _native.launch("octa_conv2d_f32_wgrad_nchw", dev, x, dy, dw.t, db.t, ws.t, nbytes - (1 if p.ws_short else 0), N, Cin, H, W, Cout, p.K, p.stride, p.pad, Ho, Wo)
    _sync()
    assert why in str(e.value), f"{name}: refused with '{e.value}', expected '{why}'"
    for buf in (y, dw, db, ws):
        assert buf.untouched(), f"{name}: a refused call wrote"


@pytest.mark.parametrize("field", ["N", "Cin", "H", "W", "Cout", "K", "stride", "pad", "Ho", "Wo"])
def test_workspace_query_refusals(hip_lib_built, field):
    """the fifth entry point: no context, no launch; a refused query leaves the caller's size untouched"""
    from octa_autosegmentation_amd import _native
    ok = dict(N=1, Cin=8, H=8, W=8, Cout=32, K=3, stride=1, pad=1, Ho=8, Wo=8)
    for v in (-1, 0):
        a = dict(ok, **{field: v})
        nbytes = ctypes.c_size_t(12345)
        if cr.workspace_refusal(**a) is None:
            _native.call("octa_conv2d_f32_wgrad_workspace", *a.values(), ctypes.byref(nbytes))
            assert nbytes.value == cr.plan_wgrad(a["N"], a["Cin"], a["Cout"], a["K"], a["stride"], a["Ho"], a["Wo"]).bytes
        else:
            with pytest.raises(_native.OctaHipError, match="octa_conv2d_f32_wgrad_workspace: bad arguments"):
                _native.call("octa_conv2d_f32_wgrad_workspace", *a.values(), ctypes.byref(nbytes))
            assert nbytes.value == 12345


# ---- exact layers through the binding ---------------------------------------------------------------------------------------------------------
# forward and all gradients in float64 on the CPU; the operands are exact-family numbers, so the float64 result is the one legal fp32 result

def _conv(gen, transposed, cin, cout, K, s, pad, bias):
    conv = (torch.nn.ConvTranspose2d(cin, cout, K, s, bias=False) if transposed else torch.nn.Conv2d(cin, cout, K, s, pad, bias=bias)).to(DEV)
    _redraw(conv, gen)
    return conv


def _redraw(conv, gen):
    """new exact-family weights IN PLACE (as an optimiser step writes them: the version counter moves, the packed copies are stale)"""
    with torch.no_grad():
        conv.weight.copy_(cr._quarters(tuple(conv.weight.shape), 2, gen, zero_half=True))
        if conv.bias is not None:
            conv.bias.copy_(cr._quarters(tuple(conv.bias.shape), 2, gen, unit=16))


def _f64_layer(conv, x, transposed):
    w = conv.weight.detach().double().cpu().requires_grad_(True)
    b = conv.bias.detach().double().cpu().requires_grad_(True) if conv.bias is not None else None
    x = x.detach().double().cpu().requires_grad_(True)
    if transposed:
        return torch.nn.functional.conv_transpose2d(x, w, stride=conv.stride), x, w, b
    return torch.nn.functional.conv2d(x, w, b, stride=conv.stride, padding=conv.padding), x, w, b


def _same(got, want64, what):
    assert got.dtype == F32 and got.shape == want64.shape, what
    assert torch.equal(want64.float().double(), want64) and torch.equal(got.detach().cpu(), want64.float()), f"{what}: not the float64 result, bit for bit"


# every kind supported() accepts: (transposed, K, stride, pad); the first five are the kinds _layer_kind accepts
LAYER_KINDS = [(0, 1, 1, 0), (0, 3, 1, 1), (0, 3, 2, 1), (1, 1, 1, 0), (1, 2, 2, 0), (0, 4, 1, 1), (0, 7, 1, 0), (0, 7, 1, 3), (0, 3, 1, 0), (0, 4, 1, 0), (0, 4, 1, 2)]


@pytest.mark.parametrize("transposed,K,s,pad", LAYER_KINDS)
def test_forward_exact_through_the_binding(hip_lib_built, transposed, K, s, pad):
    from octa_autosegmentation_amd.models import conv_f32
    gen = torch.Generator().manual_seed(700 + 10 * K + s + pad)
    cin = 2 if K == 7 else 5
    conv = _conv(gen, transposed, cin, 33, K, s, pad, bias=True)
    assert conv_f32.supported(conv)
    x = cr._quarters((2, cin, 9 + K, 67 + K), 3, gen).to(DEV)
    for _ in range(2):                                # the second round: new weights behind the same parameter, the cached pack must not be served
        with torch.no_grad():
            assert conv_f32.applies(conv, x)
            y1, y2 = conv_f32.forward(conv, x), conv_f32.forward(conv, x)          # packs, then takes the cached pack
        _sync()
        want = _f64_layer(conv, x, transposed)[0].detach()
        _same(y1, want, "y")
        assert torch.equal(_bits(y1), _bits(y2))
        _redraw(conv, gen)


@pytest.mark.parametrize("transposed,K,s,pad", LAYER_KINDS[:5])
@pytest.mark.parametrize("n,h,w,cin,cout", [(2, 9, 33, 9, 33), (1, 4, 6, 33, 5)])
def test_training_exact_through_the_binding(hip_lib_built, transposed, K, s, pad, n, h, w, cin, cout):
    from octa_autosegmentation_amd.models import conv_f32
    gen = torch.Generator().manual_seed(800 + 10 * K + s + h)
    conv = _conv(gen, transposed, cin, cout, K, s, pad, bias=True)
    assert conv_f32._layer_kind(conv) == (K, s, pad, bool(transposed))
    x = cr._quarters((n, cin, h, w), 3, gen).to(DEV).requires_grad_(True)
    for _ in range(2):
        assert conv_f32.trainable(conv, x)
        leaves = [x, conv.weight] + ([conv.bias] if conv.bias is not None else [])
        y = conv_f32.train_forward(conv, x)
        dy = cr._quarters(tuple(y.shape), 3, gen).to(DEV)
        grads = [torch.autograd.grad(y, leaves, dy, retain_graph=True) for _ in range(2)]
        _sync()
        y64, x64, w64, b64 = _f64_layer(conv, x, transposed)
        y64.backward(dy.double().cpu())
        _same(y, y64.detach(), "y")
        for g, ref, what in zip(grads[0], [x64.grad, w64.grad] + ([b64.grad] if b64 is not None else []), ("dx", "dw", "db")):
            _same(g, ref, what)
        for g0, g1 in zip(*grads):
            assert torch.equal(_bits(g0), _bits(g1)), "two backward passes differ"
        _redraw(conv, gen)
