"""GPU: the one-channel-side convolutions of the GAN networks (csrc/thin_conv.hip through models/thin_conv.py) against torch's
conv2d in fp32 on the same bf16-rounded operands: forward, data gradient, weight and bias gradients; tolerance = one bf16 rounding
of the result (outputs / dx) and fp32 summation order (dw, db).

Below those: every kernel of the file against the float64 reference of tests/_thin_ref.py (proved on the CPU by tests/test_thin_ref.py) --
exact cases bit for bit, real-valued cases inside the derived bound on every element -- through direct calls of the four entry points
with every output and the wgrad scratch between sentinels, the refusals of the host code, and exact cases through autograd. Each test
prints its error / bound ratios (RATIO lines) before it asserts them."""
import pytest
import torch

import _thin_ref as tr
from _guarded import DEV, Guarded      # the sentinel-filled buffers, shared with tests/test_conv_exact_gpu.py

pytestmark = pytest.mark.gpu


def _ref(x_nchw, conv, slope, dy_nchw):
    x = x_nchw.float().requires_grad_(True)
    w = conv.weight.detach().float().requires_grad_(True)
    b = conv.bias.detach().float().requires_grad_(True)
    with torch.backends.cudnn.flags(enabled=False):
        y = torch.nn.functional.conv2d(x, w, b, padding=conv.padding)
    if slope != 1.0:
        y = torch.nn.functional.leaky_relu(y, slope)
    y.backward(dy_nchw.float())
    return y.detach(), x.grad, w.grad, b.grad


def _close(got, want, rtol, what):
    err = (got.float() - want).abs().max().item()
    scale = want.abs().max().item()
    assert err <= rtol * scale + 1e-6, f"{what}: max error {err:.3e} vs scale {scale:.3e}"


@pytest.mark.parametrize("k,pad,c,h,w,slope", [(7, 0, 64, 70, 86, 1.0), (4, 1, 64, 61, 75, 0.2), (7, 0, 64, 310, 310, 1.0)])
def test_one_input_channel(hip_lib_built, k, pad, c, h, w, slope):
    """Generator stem (7x7 on the reflect-padded image) and discriminator stem (4x4, padding 1, LeakyReLU(0.2) fused)."""
    from octa_autosegmentation_amd.models import thin_conv
    torch.manual_seed(k * 100 + h)
    conv = torch.nn.Conv2d(1, c, k, 1, pad).cuda()
    assert thin_conv.supported(conv)
    x = torch.randn(3, 1, h, w, device="cuda").to(torch.bfloat16)
    xs = x[:, 0].clone().requires_grad_(True)
    y = thin_conv.conv_from_1(xs, conv, slope)
    dy = torch.randn(y.shape, device="cuda").to(torch.bfloat16)
    y.backward(dy)
    y_ref, dx_ref, dw_ref, db_ref = _ref(x, conv, slope, dy.permute(0, 3, 1, 2))
    _close(y.permute(0, 3, 1, 2), y_ref, 6e-3, "forward")
    _close(xs.grad[:, None], dx_ref, 6e-3, "dx")
    _close(conv.weight.grad, dw_ref, 2e-3 if slope == 1.0 else 1e-2, "dw")      # with the fused LeakyReLU dy * slope is rounded to bf16 once more
    _close(conv.bias.grad, db_ref, 2e-3 if slope == 1.0 else 1e-2, "db")


@pytest.mark.parametrize("k,pad,c,h,w", [(7, 0, 64, 70, 86), (4, 1, 512, 38, 38), (4, 1, 128, 21, 45), (7, 0, 64, 310, 310)])
def test_one_output_channel(hip_lib_built, k, pad, c, h, w):
    """Generator head (7x7, 64 -> 1) and discriminator head (4x4, 512 -> 1)."""
    from octa_autosegmentation_amd.models import thin_conv
    torch.manual_seed(k * 100 + h + c)
    conv = torch.nn.Conv2d(c, 1, k, 1, pad).cuda()
    assert thin_conv.supported(conv)
    x = torch.randn(2, c, h, w, device="cuda").to(torch.bfloat16)
    xs = x.permute(0, 2, 3, 1).contiguous().requires_grad_(True)
    y = thin_conv.conv_to_1(xs, conv)
    dy = torch.randn(y.shape, device="cuda").to(torch.bfloat16)
    y.backward(dy)
    y_ref, dx_ref, dw_ref, db_ref = _ref(x, conv, 1.0, dy[:, None])
    _close(y[:, None], y_ref, 6e-3, "forward")
    _close(xs.grad.permute(0, 3, 1, 2), dx_ref, 6e-3, "dx")
    _close(conv.weight.grad, dw_ref, 2e-3, "dw")
    _close(conv.bias.grad, db_ref, 2e-3, "db")


def test_unsupported_shapes_are_refused(hip_lib_built):
    from octa_autosegmentation_amd import _native
    from octa_autosegmentation_amd.models import thin_conv
    assert not thin_conv.supported(torch.nn.Conv2d(1, 64, 3, 1, 1))
    assert not thin_conv.supported(torch.nn.Conv2d(1, 48, 7))
    assert not thin_conv.supported(torch.nn.Conv2d(1, 64, 4, 2, 1))
    conv = torch.nn.Conv2d(1, 48, 7).cuda()
    with pytest.raises(_native.OctaHipError):
        thin_conv.conv_from_1(torch.zeros(1, 16, 16, device="cuda"), conv)


def test_lrelu_backward_kernel_equals_the_torch_expression(hip_lib_built):
    """octa_lrelu_bwd_bf16 (one launch in the backward of the expand layer with its fused LeakyReLU) against torch.where(y > 0, dy, dy * slope),
    bit for bit, including a length that is no multiple of the 8-element vectors."""
    import ctypes
    from octa_autosegmentation_amd import _native
    g = torch.Generator(device="cuda").manual_seed(5)
    for n in (8 * 1000 + 5, 3, 64 * 303 * 303):
        y = torch.randn(n, device="cuda", generator=g).to(torch.bfloat16)
        y[::17] = 0.0
        dy = torch.randn(n, device="cuda", generator=g).to(torch.bfloat16)
        out = torch.empty_like(dy)
        _native.check(_native.lib().octa_lrelu_bwd_bf16(_native.ctx(0), ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(dy.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                                       n, 0.2, _native.current_stream_ptr()), "octa_lrelu_bwd_bf16")
        assert torch.equal(out, torch.where(y > 0, dy, dy * 0.2)), n


# ---- the kernels against tests/_thin_ref.py ---------------------------------------------------------------------------------------------

def _dev(ops):
    return {k: (v.to(DEV) if v is not None else None) for k, v in ops.items()}


def _call(c, o):
    """One direct call of the entry point of case c on device operands o -> (name -> output, [Guarded])"""
    from octa_autosegmentation_amd import _native
    K = c.K
    if c.kind == "expand":
        N, Hs, Ws = o["s"].shape
        C = o["w"].shape[0]
        out = Guarded((N, Hs + 2 * c.pad - K + 1, Ws + 2 * c.pad - K + 1, C), torch.bfloat16)
        _native.launch("octa_thinconv_expand", o["s"].device, o["s"], o["w"], o["b"], out.t, N, Hs, Ws, C, K, c.pad, c.flip, float(c.slope))
        return dict(out=out.t), [out]
    N, Ha, Wa, C = o["a"].shape
    if c.kind == "squeeze":
        out = Guarded((N, Ha + 2 * c.pad - K + 1, Wa + 2 * c.pad - K + 1), torch.bfloat16)
        _native.launch("octa_thinconv_squeeze", o["a"].device, o["a"], o["w"], o["b"], out.t, N, Ha, Wa, C, K, c.pad, c.flip)
        return dict(out=out.t), [out]
    floats = int(_native.lib().octa_thinconv_wgrad_scratch_floats(N, Ha, C, K))
    assert floats == ((N * Ha + 1) // 2) * C * (K * K + 1)
    scratch, g = Guarded((floats,), torch.float32), Guarded((C, K * K), torch.float32)       # exactly the floats the library asks for
    asum = Guarded((C,), torch.float32) if c.want_asum else None
    _native.launch("octa_thinconv_wgrad", o["a"].device, o["a"], o["s"], scratch.t, g.t, asum.t if asum is not None else None,
                   N, Ha, Wa, o["s"].shape[1], o["s"].shape[2], C, K, c.pad, c.flip)
    got = dict(g=g.t)
    if asum is not None:
        got["asum"] = asum.t
    return got, [scratch, g] + ([asum] if asum is not None else [])


def _run_case(fam, name):
    for var in tr.VARIANTS:
        c = tr.case(fam, name, var)
        o = _dev(c.ops)
        r = tr.ref_of(c, o)                       # float64, on the device, from the operands the kernel gets
        got, guards = _call(c, o)
        torch.cuda.synchronize()
        rat = tr.check(c, r, got)
        print("RATIO", f"{fam}/{name}/{var}", " ".join(f"{fam}.{k}={v:.4g}" for k, v in rat.items()), f"D={c.D}")
        assert all(gd.intact() for gd in guards), f"{fam}/{name}/{var}: a sentinel around an output or the scratch was overwritten"
        if var == "exact":
            assert all(v == 0.0 for v in rat.values()), f"{fam}/{name}: not the one legal result, bit for bit ({rat})"
        else:
            assert all(v <= 1.0 for v in rat.values()), f"{fam}/{name}: error / bound above 1 ({rat}, D = {c.D})"


@pytest.mark.parametrize("name", list(tr.EXPAND_CASES))
def test_expand_kernel(hip_lib_built, name):
    _run_case("expand", name)


@pytest.mark.parametrize("name", list(tr.SQUEEZE_WIDE_CASES))
def test_squeeze_wide_kernel(hip_lib_built, name):
    _run_case("squeeze_wide", name)


@pytest.mark.parametrize("name", list(tr.SQUEEZE_LANE_CASES))
def test_squeeze_lane_per_channel_kernel(hip_lib_built, name):
    _run_case("squeeze_lane", name)


@pytest.mark.parametrize("name", list(tr.WGRAD_WIDE_CASES))
def test_wgrad_wide_kernel(hip_lib_built, name):
    _run_case("wgrad_wide", name)


@pytest.mark.parametrize("name", list(tr.WGRAD_LANE_CASES))
def test_wgrad_lane_per_channel_kernel(hip_lib_built, name):
    _run_case("wgrad_lane", name)


def _exact_ops(gen, kind, N, H, W, C, K, bias=True):
    """exact operands for a direct call: input extent H x W (expand: s, squeeze: a)"""
    shape = (N, H, W) if kind == "expand" else (N, H, W, C)
    o = {"s" if kind == "expand" else "a": tr._quarters(shape, 3, gen).to(torch.bfloat16), "w": tr._quarters((C, K * K), 2, gen, zero_half=True),
         "b": tr._quarters((C if kind == "expand" else 1,), 4, gen) if bias else None}
    return _dev(o)


def _direct(kind, o, K, pad, flip, slope=1.0, want_asum=False):
    c = tr.SimpleNamespace(kind=kind, K=K, pad=pad, flip=flip, slope=slope, want_asum=want_asum)
    got, guards = _call(c, o)
    torch.cuda.synchronize()
    assert all(gd.intact() for gd in guards)
    return got


def test_squeeze_accepts_and_refuses_what_the_mirror_of_its_dispatch_says(hip_lib_built):
    """every multiple of 64 channels up to 1024 the C ABI offers, on one K x K image (one output): wide form, lane-per-channel form, or
    the refusal when neither form's weights fit the LDS -- as tests/_thin_ref.squeeze_form reads the host code -- and the exact result"""
    from octa_autosegmentation_amd import _native
    gen = torch.Generator().manual_seed(77)
    seen = set()
    for K in (4, 7):
        for C in range(64, 1025, 64):
            o = _exact_ops(gen, "squeeze", 2, K, K + 1, C, K)
            form = tr.squeeze_form(C, K)
            seen.add(form)
            if form is None:
                with pytest.raises(_native.OctaHipError):
                    _direct("squeeze", o, K, 0, 1)
                continue
            r = tr.reference("squeeze", K, 0, 1, **o)
            assert r.S.max().item() < tr.EXACT_LIMIT
            assert torch.equal(_direct("squeeze", o, K, 0, 1)["out"], tr.once(r.out)), (K, C, form)
    assert seen == {"wide", "lane", None}


def test_expand_at_the_widest_row_the_lds_window_takes_and_its_refusal_one_pixel_wider(hip_lib_built):
    from octa_autosegmentation_amd import _native
    gen = torch.Generator().manual_seed(78)
    K, Wo = 4, 3821                                  # (64 * 17 + 4 * (Wo + 3)) * 4 bytes = 64 KB exactly
    assert tr.expand_ok(64, K, Wo) and not tr.expand_ok(64, K, Wo + 1)
    o = _exact_ops(gen, "expand", 1, 3, Wo + 1, 64, K)
    r = tr.reference("expand", K, 1, 0, slope=0.25, **o)
    assert torch.equal(_direct("expand", o, K, 1, 0, 0.25)["out"], tr.once(r.out))
    o = _exact_ops(gen, "expand", 1, 3, Wo + 2, 64, K)
    with pytest.raises(_native.OctaHipError, match="LDS"):
        _direct("expand", o, K, 1, 0, 0.25)


def test_refusals(hip_lib_built):
    """Each call gets buffers of the full size it would need, so that a missing refusal is a wrong answer and not an out-of-bounds access."""
    from octa_autosegmentation_amd import _native
    gen = torch.Generator().manual_seed(79)

    def refused(kind, N, H, W, C, K, pad, match):
        KK = K * K
        a = tr._quarters((N, H, W, C), 3, gen).to(torch.bfloat16).to(DEV)
        s = tr._quarters((N, H + 2 * K, W + 2 * K), 3, gen).to(torch.bfloat16).to(DEV)
        w, b = torch.ones((C, KK), device=DEV), torch.ones(C, device=DEV)
        out = Guarded((N, H + 2 * K, W + 2 * K, C), torch.bfloat16)                      # larger than any output extent of the call
        scratch = Guarded((max(1, ((N * H + 1) // 2) * C * (KK + 1)),), torch.float32)
        g, asum = Guarded((C, KK), torch.float32), Guarded((C,), torch.float32)
        with pytest.raises(_native.OctaHipError, match=match):
            if kind == "expand":
                _native.launch("octa_thinconv_expand", s.device, s[:, :H, :W].contiguous(), w, b, out.t, N, H, W, C, K, pad, 0, 1.0)
            elif kind == "squeeze":
                _native.launch("octa_thinconv_squeeze", a.device, a, w, b, out.t, N, H, W, C, K, pad, 0)
            else:
                _native.launch("octa_thinconv_wgrad", a.device, a, s, scratch.t, g.t, asum.t, N, H, W, s.shape[1], s.shape[2], C, K, pad, 0)
        torch.cuda.synchronize()
        for buf in (out, scratch, g, asum):
            assert bool((buf.raw == buf.pattern).all()), "a refused call wrote"

    for kind in ("expand", "squeeze", "wgrad"):
        refused(kind, 1, 9, 9, 48, 4, 1, "multiple of 64")
        refused(kind, 1, 9, 9, 1088, 4, 1, "multiple of 64")
        refused(kind, 1, 9, 9, 64, 5, 1, "unsupported shape")
        refused(kind, 1, 9, 9, 64, 4, 4, "unsupported shape")
        refused(kind, 1, 9, 9, 64, 7, 7, "unsupported shape")
    for kind in ("expand", "squeeze"):                                                   # no window fits: H + 2 pad < K
        refused(kind, 1, 4, 9, 64, 7, 1, "unsupported shape")
        refused(kind, 1, 9, 1, 64, 4, 1, "unsupported shape")
    refused("squeeze", 1, 2, 9, 64, 3, 0, "K = 3")
    refused("squeeze", 1, 9, 9, 128, 3, 1, "K = 3")
    refused("squeeze", 1, 9, 9, 512, 7, 3, "do not fit the LDS")                         # neither form's weight table fits
    refused("squeeze", 1, 9, 9, 1024, 4, 1, "do not fit the LDS")


@pytest.mark.parametrize("n", [1, 7, 8, 9, 8 * 300 + 3])
def test_lrelu_backward_kernel_on_short_lengths_signed_zero_and_subnormals(hip_lib_built, n):
    """out = y > 0 ? dy : bf16(dy * slope) against the same expression on the CPU in fp32, bit for bit: y with -0.0, +0.0 and bf16
    subnormals of either sign (positive ones take the dy branch), dy with subnormals (dy * slope is an fp32 subnormal), the n % 8 tail
    alone (n < 8), and the refusal of a tensor that is not 16-byte aligned."""
    from octa_autosegmentation_amd import _native
    gen = torch.Generator().manual_seed(100 + n)
    y = torch.randn(n + 1, generator=gen).to(torch.bfloat16)
    dy = torch.randn(n + 1, generator=gen).to(torch.bfloat16)
    special = torch.tensor([-0.0, 0.0, 9.1835e-41, -9.1835e-41, 1.1663e-38, -1.1663e-38, 1e-39], dtype=torch.float32).to(torch.bfloat16)
    idx = torch.arange(n + 1)
    y[::2] = special[(idx[::2] // 2) % 7]
    dy[1::3] = special[(idx[1::3] // 3 + 2) % 7]
    assert n < 2 or ((y.float() == 0) & (y.view(torch.int16) < 0)).any()       # a -0.0 is there
    slope = 0.2
    yd, dyd = y.to(DEV), dy.to(DEV)
    out = Guarded((n,), torch.bfloat16)
    _native.launch("octa_lrelu_bwd_bf16", yd.device, yd[:n], dyd[:n], out.t, n, slope)
    torch.cuda.synchronize()
    want = torch.where(y.float() > 0, dy.float(), dy.float() * torch.tensor(slope, dtype=torch.float32)).to(torch.bfloat16)[:n]
    assert out.intact()
    assert torch.equal(out.t.cpu().view(torch.int16), want.view(torch.int16)), n       # the bits: -0.0 * slope is -0.0
    for bad in ((yd[1:], dyd[:n], out.t), (yd[:n], dyd[1:], out.t)):
        with pytest.raises(_native.OctaHipError, match="16-byte aligned"):
            _native.launch("octa_lrelu_bwd_bf16", yd.device, *bad, n, slope)
    if n > 1:
        with pytest.raises(_native.OctaHipError, match="16-byte aligned"):
            _native.launch("octa_lrelu_bwd_bf16", yd.device, yd[:n - 1], dyd[:n - 1], out.t[1:], n - 1, slope)


# ---- exact cases through autograd ----------------------------------------------------------------------------------------------------------

def _exact_conv(gen, cin, cout, k, pad, bias=True):
    conv = torch.nn.Conv2d(cin, cout, k, 1, pad, bias=bias)
    with torch.no_grad():
        conv.weight.copy_(tr._quarters(tuple(conv.weight.shape), 2, gen, zero_half=True))
        if bias:
            conv.bias.copy_(tr._quarters((cout,), 4, gen))
    return conv


def _f64_autograd(x_nchw, conv, slope, dy_nchw):
    """y, dx, dw, db of the layer in float64 on the CPU (every operand exact: so is every sum)"""
    x = x_nchw.double().cpu().requires_grad_(True)
    w = conv.weight.detach().double().cpu().requires_grad_(True)
    b = conv.bias.detach().double().cpu().requires_grad_(True) if conv.bias is not None else None
    y = torch.nn.functional.conv2d(x, w, b, padding=conv.padding)
    y = torch.where(y > 0, y, y * slope)
    y.backward(dy_nchw.double().cpu())
    return y.detach(), x.grad, w.grad, (b.grad if b is not None else None)


def _backward_twice(y, dy, leaves):
    """-> the gradients of `leaves`; the backward runs twice and has to give identical bits (wgrad: per-block partial sums, one reduction)"""
    runs = []
    for _ in range(2):
        for t in leaves:
            t.grad = None
        y.backward(dy, retain_graph=True)
        torch.cuda.synchronize()
        runs.append([t.grad.clone() for t in leaves])
    for t, g0, g1 in zip(leaves, runs[0], runs[1]):
        assert torch.equal(g0.view(torch.int16 if g0.dtype == torch.bfloat16 else torch.int32), g1.view(torch.int16 if g1.dtype == torch.bfloat16 else torch.int32)), \
            "two backward passes differ"
    return runs[0]


def _same(got, want64, what):
    want = tr.once(want64) if got.dtype == torch.bfloat16 else want64.float()
    assert torch.equal(got.cpu().reshape(want.shape), want), f"{what}: not the float64 result rounded once"


# k, pad, c, n, h, w, slope: the generator's and the discriminator's stem; Ho = 1 (H = K at pad 0); 512 channels
@pytest.mark.parametrize("k,pad,c,n,h,w,slope", [(7, 0, 64, 2, 9, 12, 1.0), (4, 1, 64, 3, 6, 7, 0.25), (7, 0, 64, 2, 7, 10, 0.25), (4, 1, 512, 1, 5, 6, 0.25),
                                                 (4, 0, 128, 2, 5, 4, 1.0)])
def test_conv_from_1_exact_through_autograd(hip_lib_built, k, pad, c, n, h, w, slope):
    from octa_autosegmentation_amd.models import thin_conv
    gen = torch.Generator().manual_seed(k * 1000 + c + h)
    conv = _exact_conv(gen, 1, c, k, pad).to(DEV)
    assert thin_conv.supported(conv)
    x = tr._quarters((n, 1, h, w), 3, gen).to(torch.bfloat16)
    xs = x[:, 0].to(DEV).requires_grad_(True)
    y = thin_conv.conv_from_1(xs, conv, slope)
    dy = tr._quarters(tuple(y.shape), 3, gen).to(torch.bfloat16).to(DEV)
    dx, dw, db = _backward_twice(y, dy, [xs, conv.weight, conv.bias])
    y_ref, dx_ref, dw_ref, db_ref = _f64_autograd(x, conv, slope, dy.permute(0, 3, 1, 2))
    _same(y.detach().permute(0, 3, 1, 2), y_ref, "y")
    _same(dx[:, None], dx_ref, "dx")
    _same(dw, dw_ref, "dw")
    _same(db, db_ref, "db")


@pytest.mark.parametrize("k,pad,c,n,h,w", [(7, 0, 64, 2, 9, 12), (4, 1, 512, 1, 5, 7), (4, 1, 128, 3, 3, 4), (7, 3, 256, 1, 7, 9), (7, 0, 64, 2, 7, 7)])
def test_conv_to_1_exact_through_autograd(hip_lib_built, k, pad, c, n, h, w):
    from octa_autosegmentation_amd.models import thin_conv
    gen = torch.Generator().manual_seed(k * 1000 + c + h + 1)
    conv = _exact_conv(gen, c, 1, k, pad).to(DEV)
    assert thin_conv.supported(conv)
    x = tr._quarters((n, c, h, w), 3, gen).to(torch.bfloat16)
    xs = x.permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(True)
    y = thin_conv.conv_to_1(xs, conv)
    dy = tr._quarters(tuple(y.shape), 3, gen).to(torch.bfloat16).to(DEV)
    dx, dw, db = _backward_twice(y, dy, [xs, conv.weight, conv.bias])
    y_ref, dx_ref, dw_ref, db_ref = _f64_autograd(x, conv, 1.0, dy[:, None])
    _same(y.detach()[:, None], y_ref, "y")
    _same(dx.permute(0, 3, 1, 2), dx_ref, "dx")
    _same(dw, dw_ref, "dw")
    _same(db, db_ref, "db")


@pytest.mark.parametrize("cout,n,h,w", [(8, 2, 6, 7), (16, 2, 3, 4), (32, 1, 4, 5), (64, 1, 5, 9)])
def test_conv3x3_one_channel_data_gradient_exact_through_autograd(hip_lib_built, cout, n, h, w):
    """the segmentor's one-channel 3 x 3 first layer (mfma_conv.conv3x3): its data gradient is the K = 3 form of the wide squeeze kernel"""
    from octa_autosegmentation_amd.models import mfma_conv
    gen = torch.Generator().manual_seed(3000 + cout)
    conv = _exact_conv(gen, 1, cout, 3, 1, bias=False).to(DEV)
    x = tr._quarters((n, 1, h, w), 3, gen).to(torch.bfloat16)
    xs = x.permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(True)
    y = mfma_conv.conv3x3(xs, conv.weight)
    assert y.shape == (n, h, w, cout)
    dy = tr._quarters(tuple(y.shape), 3, gen).to(torch.bfloat16).to(DEV)
    dx, dw = _backward_twice(y, dy, [xs, conv.weight])
    y_ref, dx_ref, dw_ref, _ = _f64_autograd(x, conv, 1.0, dy.permute(0, 3, 1, 2))
    _same(y.detach().permute(0, 3, 1, 2), y_ref, "y")
    _same(dx.permute(0, 3, 1, 2), dx_ref, "dx")
    _same(dw, dw_ref, "dw")
