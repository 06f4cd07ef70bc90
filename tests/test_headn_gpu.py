"""GPU: the 1x1 convolution head to N channels on the matrix cores (csrc/head.hip), its autograd binding, the DynUNet that ends in it
and the fused Dice + BCE loss on several channels."""
import pytest

pytestmark = pytest.mark.gpu

GUARD = 67            # odd: the channel-first buffers start at 2-byte alignment only
GUARD8 = 64           # dx is written in 8-byte pieces: its guard keeps the allocation's alignment
SENT16, SENT32 = 0x7A5C, 12345.678


def _guarded(numel, dtype, guard, sentinel):
    import torch
    buf = torch.full((numel + 2 * guard,), sentinel, dtype=dtype, device="cuda")
    return buf, buf[guard:guard + numel]


def _intact(buf, numel, guard, sentinel):
    import torch
    want = torch.full((guard,), sentinel, dtype=buf.dtype, device=buf.device)
    return bool(torch.equal(buf[:guard], want)) and bool(torch.equal(buf[guard + numel:], want))


def _check(got, want):
    """tests/test_conv_gpu.py's bound: 2^-8 of the tensor's scale (one bf16 rounding of an fp32 sum)."""
    err = (got.float() - want).abs()
    scale = want.abs().max().item() + 1e-6
    print("max err", err.max().item(), "scale", scale)
    assert err.max().item() <= scale * 2.0 ** -8 + 1e-6, (err.max().item(), scale)


def _case(n, h, w, cin, cout, bias):
    import torch
    g = torch.Generator(device="cuda").manual_seed(1000 * h + 10 * cout + cin)
    x = torch.randn(n, h * w, cin, device="cuda", generator=g).to(torch.bfloat16)
    # asymmetric weights and distinct biases: a swapped channel or a transposed tile cannot pass
    wt = (torch.randn(cout, cin, device="cuda", generator=g) * 0.2).to(torch.bfloat16).float()
    b = (torch.randn(cout, device="cuda", generator=g) + torch.arange(cout, device="cuda") * 0.05) if bias else None
    dy = torch.randn(n, cout, h * w, device="cuda", generator=g).to(torch.bfloat16)
    return x, wt, b, dy


def _launch_bwd(x, dyv, wt, n, hw, cin, cout, want_db):
    import torch
    from octa_autosegmentation_amd import _native
    dx_buf, dx = _guarded(n * hw * cin, torch.int16, GUARD8, SENT16)
    dw_buf, dw = _guarded(cout * cin, torch.float32, GUARD, SENT32)
    db_buf, db = _guarded(cout, torch.float32, GUARD, SENT32)
    _native.launch("octa_headn_nhwc_bwd", x.device, x, dyv, wt, n, hw, cin, cout, dx, dw, db if want_db else None)
    torch.cuda.synchronize()
    return (dx_buf, dx), (dw_buf, dw), (db_buf, db)


CASES = [
    (2, 37, 53, 32, 44, True),     # odd hw, a partial last channel tile, tiles that straddle images
    (1, 5, 3, 32, 2, True),        # fewer pixels than one tile, fewer channels than one tile
    (2, 16, 64, 64, 16, True),     # exact tiles
    (1, 33, 31, 64, 64, True),     # the maximum Cout
    (3, 7, 5, 32, 20, False),      # no bias; several images inside one tile
]


@pytest.mark.parametrize("n,h,w,cin,cout,bias", CASES)
def test_kernels_match_fp32_torch(hip_lib_built, n, h, w, cin, cout, bias):
    import torch
    from octa_autosegmentation_amd import _native
    x, wt, b, dy = _case(n, h, w, cin, cout, bias)
    hw = h * w
    y_ref = torch.einsum("nqc,oc->noq", x.float(), wt) + (b.view(1, cout, 1) if bias else 0.0)
    dx_ref = torch.einsum("noq,oc->nqc", dy.float(), wt)
    dw_ref = torch.einsum("noq,nqc->oc", dy.float(), x.float())
    db_ref = dy.float().sum((0, 2))

    y_buf, y = _guarded(n * cout * hw, torch.int16, GUARD, SENT16)
    _native.launch("octa_headn_nhwc_fwd", x.device, x, wt, b, n, hw, cin, cout, y)
    torch.cuda.synchronize()
    assert _intact(y_buf, n * cout * hw, GUARD, SENT16)
    _check(y.view(torch.bfloat16).view(n, cout, hw), y_ref)

    # dy at an odd element offset too: the unaligned row reads
    dy_buf, dyv = _guarded(n * cout * hw, torch.int16, GUARD, SENT16)
    dyv.copy_(dy.view(torch.int16).reshape(-1))
    (dx_buf, dx), (dw_buf, dw), (db_buf, db) = _launch_bwd(x, dyv, wt, n, hw, cin, cout, bias)
    assert _intact(dx_buf, n * hw * cin, GUARD8, SENT16) and _intact(dw_buf, cout * cin, GUARD, SENT32) and _intact(db_buf, cout, GUARD, SENT32)
    _check(dx.view(torch.bfloat16).view(n, hw, cin), dx_ref)
    e_dw, s_dw = (dw.view(cout, cin) - dw_ref).abs().max().item(), dw_ref.abs().max().item()
    print("dw err", e_dw, "largest", s_dw)
    assert e_dw <= s_dw * 1e-3
    if bias:
        e_db, s_db = (db - db_ref).abs().max().item(), db_ref.abs().max().item()
        print("db err", e_db, "largest", s_db)
        assert e_db <= s_db * 1e-3
    else:
        assert bool((db == SENT32).all())          # NULL d_db: nothing written


def test_backward_is_bit_identical_between_runs(hip_lib_built):
    import torch
    n, h, w, cin, cout = 2, 37, 53, 32, 44
    x, wt, _, dy = _case(n, h, w, cin, cout, True)
    dyv = dy.view(torch.int16).reshape(-1)
    runs = [_launch_bwd(x, dyv, wt, n, h * w, cin, cout, True) for _ in range(2)]
    for (_, a), (_, b) in zip(*runs):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


def test_unsupported_shapes_are_refused(hip_lib_built):
    import torch
    from octa_autosegmentation_amd import _native
    x = torch.zeros(1, 16, 48, dtype=torch.bfloat16, device="cuda")
    y = torch.zeros(1, 65, 16, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(65, 48, device="cuda")
    for cin, cout in ((48, 4), (32, 65), (32, 1)):
        with pytest.raises(_native.OctaHipError, match="unsupported shape"):
            _native.launch("octa_headn_nhwc_fwd", x.device, x, w, None, 1, 16, cin, cout, y)


def test_binding_returns_channel_first_and_its_gradients(hip_lib_built):
    import torch
    from octa_autosegmentation_amd.models import mfma_conv
    n, h, w, cin, cout = 2, 9, 11, 32, 5
    x, wt, b, dy = _case(n, h, w, cin, cout, True)
    xm = x.view(n, h, w, cin).clone().requires_grad_(True)
    wm, bm = wt.view(cout, cin, 1, 1).clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = mfma_conv.conv1x1_bias_nhwc(xm, wm, bm)
    assert y.shape == (n, cout, h, w) and y.is_contiguous() and y.dtype == torch.bfloat16
    y.backward(dy.view(n, cout, h, w))
    xr, wr, br = x.float().requires_grad_(True), wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = torch.einsum("nqc,oc->noq", xr, wr) + br.view(1, cout, 1)
    yr.backward(dy.float())
    _check(y.detach().view(n, cout, h * w), yr.detach())
    _check(xm.grad.view(n, h * w, cin), xr.grad)
    assert wm.grad.shape == wm.shape and (wm.grad.view(cout, cin) - wr.grad).abs().max().item() <= wr.grad.abs().max().item() * 1e-3
    assert (bm.grad - br.grad).abs().max().item() <= br.grad.abs().max().item() * 1e-3


def test_dynunet_with_44_channels_runs_on_own_kernels(hip_lib_built, monkeypatch):
    """DynUNet(2, 1, 44) at 2 x 1 x 64 x 96 under bf16 autocast and OCTA_STRICT=1, forward and backward: no vendor kernel, contiguous
    [2, 44, 64, 96] logits. Reference: the same network inside networks.vendor_reference(), where only the head differs (the old
    bf16 GEMM + bias, two roundings; everything upstream is the same kernels).
      logits: 3 * 2^-9 of the logits' scale (two roundings there, one here).
      output block's gradients: 1e-3 of their largest entry against the fp32 products of the tensors the head itself saw (its input
        and the gradient of its output, captured in this run) -- the reference run's own weight gradient is a bf16 GEMM output
        (rounded to 8 bits: up to 2^-8 of the largest entry), so it cannot carry a 1e-3 bound; the distance to it is printed.
        Measured: weight 2.1e-9 from the fp32 products and 7.5e-6 from the reference run at a largest entry of 2.4e-3 (3.1e-3 of it),
        bias 4.7e-10 and 9.0e-6 at 5.0e-3 (1.8e-3 of it).
      other parameters: cosine >= 0.999 with the reference run's gradients (measured worst: 0.99986, input_block.norm1.weight)."""
    import torch
    from octa_autosegmentation_amd.models import mfma_conv, networks
    from octa_autosegmentation_amd.models.losses import DiceBCELoss
    monkeypatch.setenv("OCTA_STRICT", "1")
    torch.manual_seed(11)
    net = networks.DynUNet(2, 1, 44, [3, 3, 3, 3, 3], [1, 2, 2, 2, 1], [1, 2, 2, 2, 1]).cuda()
    networks.init_weights(net, "kaiming")
    with torch.no_grad():
        net.output_block.conv.conv.bias.copy_(torch.linspace(-0.5, 0.5, 44))
    x = torch.rand(2, 1, 64, 96, device="cuda")
    tgt = (torch.rand(2, 44, 64, 96, device="cuda") > 0.7).float()
    loss_fn = DiceBCELoss(True)
    seen = {}
    plain_head = mfma_conv.conv1x1_bias_nhwc

    def spying_head(xh, weight, bias):
        y = plain_head(xh, weight, bias)
        if y.requires_grad and mfma_conv.headn_ok(xh.shape[-1], weight):
            seen["x"] = xh.detach()
            y.register_hook(lambda g: seen.__setitem__("dy", g.detach()))
        return y

    monkeypatch.setattr(mfma_conv, "conv1x1_bias_nhwc", spying_head)

    def run():
        net.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = net(x)
        loss_fn(out, tgt).backward()
        return out, {k: p.grad.float().clone() for k, p in net.named_parameters()}

    vendor0 = networks.PATH_COUNTS["vendor"]
    out, grads = run()
    assert networks.PATH_COUNTS["vendor"] == vendor0
    assert out.shape == (2, 44, 64, 96) and out.is_contiguous() and out.dtype == torch.bfloat16
    with networks.vendor_reference():
        ref_out, ref_grads = run()
    assert ref_out.shape == out.shape

    scale = ref_out.float().abs().max().item()
    e = (out.float() - ref_out.float()).abs().max().item()
    print("logits: max difference", e, "scale", scale, "bound", 3 * 2.0 ** -9 * scale)
    assert e <= 3 * 2.0 ** -9 * scale

    xh, dyh = seen["x"].float().reshape(-1, 32), seen["dy"].float().reshape(2, 44, -1)
    wb = net.output_block.conv.conv.weight
    dw_ref = torch.einsum("noq,nqc->oc", dyh, xh.view(2, -1, 32)).view_as(wb)
    db_ref = dyh.sum((0, 2))
    for name, want in (("output_block.conv.conv.weight", dw_ref), ("output_block.conv.conv.bias", db_ref)):
        got, largest = grads[name], want.abs().max().item()
        print(name, "max difference to the fp32 products", (got - want).abs().max().item(), "to the reference run", (got - ref_grads[name]).abs().max().item(),
              "largest entry", largest)
        assert (got - want).abs().max().item() <= 1e-3 * largest

    def cos(u, v):
        return (torch.dot(u, v) / (u.norm() * v.norm() + 1e-30)).item()

    worst = min((cos(grads[k].flatten(), ref_grads[k].flatten()), k) for k in grads if not k.startswith("output_block") and ref_grads[k].norm().item() > 1e-12)
    print("worst cosine of the other parameters' gradients", worst)
    assert worst[0] >= 0.999, worst


def _torch_dice_bce(x, y):
    """DiceBCELoss(sigmoid=True) as the torch expression: MONAI's Dice (mean over (sample, channel)) + BCEWithLogits (mean over all), / 2."""
    import torch
    p = torch.sigmoid(x)
    dims = tuple(range(2, x.dim()))
    dice = torch.mean(1.0 - (2.0 * torch.sum(p * y, dim=dims) + 1e-5) / (torch.sum(p, dim=dims) + torch.sum(y, dim=dims) + 1e-5))
    return (dice + torch.nn.functional.binary_cross_entropy_with_logits(x, y)) / 2


@pytest.mark.parametrize("shape", [(2, 3, 17, 19), (1, 44, 8, 8)])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_fused_loss_on_several_channels(hip_lib_built, shape, dtype):
    """The project's yardstick: the fused loss and its gradient may be at most 4x as far from the float64 evaluation of the torch
    expression as torch's own evaluation in the input dtype is (same, already rounded, input values)."""
    import torch
    from octa_autosegmentation_amd.models.losses import DiceBCELoss
    dt = getattr(torch, dtype)
    g = torch.Generator(device="cuda").manual_seed(shape[1])
    x = (torch.randn(shape, device="cuda", generator=g) * 2).to(dt)
    y = (torch.rand(shape, device="cuda", generator=g) > 0.7).float()

    def run(fn, xin, yin):
        xin = xin.clone().requires_grad_(True)
        loss = fn(xin, yin)
        loss.backward()
        return loss.detach().double().item(), xin.grad.double()

    l64, g64 = run(_torch_dice_bce, x.double(), y.double())
    l_t, g_t = run(_torch_dice_bce, x, y.to(dt))
    l_f, g_f = run(DiceBCELoss(True), x, y)
    dev_t = (abs(l_t - l64), (g_t - g64).abs().max().item())
    dev_f = (abs(l_f - l64), (g_f - g64).abs().max().item())
    print("loss deviation: torch", dev_t[0], "fused", dev_f[0], "| dx deviation: torch", dev_t[1], "fused", dev_f[1])
    assert dev_f[0] <= 4 * dev_t[0]
    assert dev_f[1] <= 4 * dev_t[1]
