"""Single-precision convolutions on the matrix cores (csrc/conv_f32.hip, `octa_conv2d_f32_nchw`) for the reference's paths that run
WITHOUT mixed precision: test.py:79 / validate.py evaluate `model.inference` outside autocast, so DynUNet's torch.nn.Conv2d /
ConvTranspose2d layers (models/networks.py:6 -> MONAI) compute in fp32 there.

`General.amp: false` training (this project maps it to plain fp32) runs the same layers through `ConvF32Train`, an autograd Function
whose forward is `forward` below and whose backward runs the exact-fp32 data-gradient (`octa_conv2d_f32_dgrad_nchw`: the forward
kernel on dy with re-packed weights; a 3x3 stride-2 layer as four output-parity classes) and weight-gradient kernels
(`octa_conv2d_f32_wgrad_nchw`: per-chunk partials in a workspace the binding allocates as a torch tensor after asking
`octa_conv2d_f32_wgrad_workspace` for its size, added in a fixed order -- bit-identical from run to run). `applies` keeps meaning
"gradient-free fp32 forward"; `trainable` says which grad-recording passes the Function covers.

Weights are re-laid-out once per weight version as [Cin][K*K][Cout] (output channel innermost: the kernel's weight slice loads are
then contiguous); a 2x2 stride-2 transposed convolution is one launch on the packed tensor [Cin][4][Cout]
(`octa_convtranspose2x2_f32_nchw`)."""
import ctypes

import torch

from .. import _native
from . import weight_cache


def fwd_layout(w, transposed):
    """The forward weight layout of `octa_conv2d_f32_nchw` (pure torch, any device): input channel outermost, output channel innermost."""
    if transposed:          # [Cin][Cout][k][k] -> [Cin][k*k][Cout]
        return w.permute(0, 2, 3, 1).reshape(w.shape[0], w.shape[2] * w.shape[3], w.shape[1]).contiguous()
    return w.permute(1, 2, 3, 0).reshape(w.shape[1], w.shape[2] * w.shape[3], w.shape[0]).contiguous()      # [Cout][Cin][K][K] -> [Cin][K*K][Cout]


def _packed(weight, transposed):
    """`fwd_layout` of the parameter, cached on it (weight_cache.cached; the orientation is part of the key)."""
    return weight_cache.cached(weight, "_octa_fwd_f32", transposed, lambda: fwd_layout(weight.detach().float(), transposed))


def _launch(x, wp, wp_offset, bias, y, Cout, cout_w, K, stride, pad, Ho, Wo, osc=1, ooy=0, oox=0):
    N, Cin, H, W = x.shape
    _native.launch("octa_conv2d_f32_nchw", x.device, x, wp.data_ptr() + 4 * wp_offset, bias, y,
                   N, Cin, H, W, Cout, cout_w, K, stride, pad, Ho, Wo, osc, ooy, oox)


def _geometry(conv):
    """(K, stride, pad, transposed) of an ungrouped, undilated layer with square kernel / stride / padding -- a zero-padded Conv2d, or a
    ConvTranspose2d with kernel == stride in (1, 2), no padding and no bias -- else None."""
    if conv.groups != 1 or tuple(conv.dilation) != (1, 1):
        return None
    k, s, p = tuple(conv.kernel_size), tuple(conv.stride), tuple(conv.padding)
    if k[0] != k[1] or s[0] != s[1] or p[0] != p[1]:
        return None
    if isinstance(conv, torch.nn.ConvTranspose2d):
        ok = k == s and k[0] in (1, 2) and p == (0, 0) and tuple(conv.output_padding) == (0, 0) and conv.bias is None
        return (k[0], s[0], 0, True) if ok else None
    if isinstance(conv, torch.nn.Conv2d) and conv.padding_mode == "zeros":
        return (k[0], s[0], p[0], False)
    return None


def supported(conv):
    """torch.nn.Conv2d / ConvTranspose2d layers this path evaluates (everything DynUNet-S holds)."""
    geom = _geometry(conv)
    if geom is None:
        return False
    K, s, pad, transposed = geom
    # zero padding up to half the kernel: DynUNet's "same" layers, the GAN networks' 3x3 / 7x7 layers behind a reflection pad (padding 0)
    # and PatchGAN's 4x4 layers with padding 1
    return transposed or ((K, s) in ((1, 1), (3, 1), (3, 2), (4, 1), (7, 1)) and 0 <= pad <= K // 2)


def applies(conv, x):
    """The fp32 matrix-core path takes a call when it is plain fp32 on the GPU and no gradient is recorded."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and supported(conv)):
        return False
    if torch.is_autocast_enabled():
        return False
    return not (torch.is_grad_enabled() and (x.requires_grad or conv.weight.requires_grad))


def forward(conv, x):
    """conv(x) for a supported layer: fp32 in, fp32 out, NCHW."""
    x = x.contiguous()
    N, Cin, H, W = x.shape
    if isinstance(conv, torch.nn.ConvTranspose2d):
        k, Cout = conv.kernel_size[0], conv.out_channels
        wp = _packed(conv.weight, True)
        y = torch.empty((N, Cout, H * k, W * k), dtype=torch.float32, device=x.device)
        if k == 2:          # one launch, both output parities of a row pair written as 8-byte pairs
            _native.launch("octa_convtranspose2x2_f32_nchw", x.device, x, wp, y, N, Cin, H, W, Cout)
            return y
        for a in range(k):
            for b in range(k):
                _launch(x, wp, (a * k + b) * Cout, None, y, Cout, k * k * Cout, 1, 1, 0, H, W, k, a, b)
        return y
    K, s, Cout = conv.kernel_size[0], conv.stride[0], conv.out_channels
    pad = conv.padding[0]
    Ho, Wo = (H + 2 * pad - K) // s + 1, (W + 2 * pad - K) // s + 1
    wp = _packed(conv.weight, False)
    bias = conv.bias.detach().float().contiguous() if conv.bias is not None else None
    y = torch.empty((N, Cout, Ho, Wo), dtype=torch.float32, device=x.device)
    _launch(x, wp, 0, bias, y, Cout, Cout, K, s, pad, Ho, Wo)
    return y


# ---- training: data and weight gradients ------------------------------------------------------------------------------------------

def _layer_kind(conv):
    """(K, stride, pad, transposed) of a layer the gradient kernels cover, else None: every layer kind of DynUNet-S."""
    geom = _geometry(conv)
    return geom if geom is not None and (geom[3] or geom[:3] in ((1, 1, 0), (3, 1, 1), (3, 2, 1))) else None


def trainable(conv, x):
    """The exact-fp32 training path takes a call when it is plain fp32 on the GPU, records a gradient and the layer is covered
    (Conv2d 1x1 / 3x3 stride 1 / 3x3 stride 2, with or without bias; ConvTranspose2d 1x1 and 2x2 stride 2 without bias)."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and conv.weight.dtype == torch.float32):
        return False
    if torch.is_autocast_enabled() or not torch.is_grad_enabled():
        return False
    if not (x.requires_grad or conv.weight.requires_grad or (conv.bias is not None and conv.bias.requires_grad)):
        return False
    return _layer_kind(conv) is not None


# stride-2 parity class a -> weight row of its tap t (t = 0: dy(i), t = 1: dy(i + 1)); None: the padded zero tap
_PARITY_TAPS = {0: (1, None), 1: (2, 0)}


def dgrad_layout(w, kind):
    """The data-gradient weight layout of `octa_conv2d_f32_dgrad_nchw` (pure torch, any device): the weights of the product that maps
    dy to dx, output (= the layer's input) channel innermost. kind = (K, stride, pad, transposed) from `_layer_kind`."""
    K, s, _, transposed = kind
    if transposed:          # w [Cin][Cout][k][k] -> [Cout][k*k][Cin]: dx = a k x k stride-k convolution of dy
        return w.permute(1, 2, 3, 0).reshape(w.shape[1], K * K, w.shape[0]).contiguous()
    cout, cin = w.shape[0], w.shape[1]
    if s == 1:              # w [Cout][Cin][K][K] -> [Cout][K*K][Cin] with flipped taps: dx = conv(dy, padding K - 1 - pad)
        return w.flip(2, 3).permute(0, 2, 3, 1).reshape(cout, K * K, cin).contiguous()
    # 3x3 stride 2 pad 1: [parity 2a + b][Cout][tap 2t + u][Cin], dx(2i + a, 2j + b) = sum_{t, u} dy(i + t, j + u) wd[2a + b][:, 2t + u]
    wd = w.new_zeros(4, cout, 4, cin)
    for a in range(2):
        for b in range(2):
            for t, r in enumerate(_PARITY_TAPS[a]):
                for u, c in enumerate(_PARITY_TAPS[b]):
                    if r is not None and c is not None:
                        wd[2 * a + b, :, 2 * t + u, :] = w[:, :, r, c]
    return wd


def _packed_dgrad(weight, kind):
    """`dgrad_layout` of the parameter, cached on it like `_packed` under its own slot: the forward and the data-gradient orientations
    do not evict each other; Adam's in-place step bumps the version, so each step repacks once."""
    return weight_cache.cached(weight, "_octa_dgrad_f32", kind, lambda: dgrad_layout(weight.detach().float(), kind))


def dgrad(conv, gy, x_shape):
    """dL/dx of a covered layer from dL/dy (fp32 NCHW)."""
    kind = _layer_kind(conv)
    K, s, pad, transposed = kind
    N, Cin, H, W = x_shape
    Cout, Ho, Wo = gy.shape[1], gy.shape[2], gy.shape[3]
    wd = _packed_dgrad(conv.weight, kind)
    dx = torch.empty((N, Cin, H, W), dtype=torch.float32, device=gy.device)
    _native.launch("octa_conv2d_f32_dgrad_nchw", gy.device, gy, wd, dx, N, Cin, H, W, Cout, K, s, pad, Ho, Wo, int(transposed))
    return dx


def wgrad(conv, x, gy, want_bias):
    """(dL/dW in the parameter's layout, dL/db or None) of a covered layer. A transposed layer's weight gradient is the same product
    with x and dy swapped."""
    K, s, pad, transposed = _layer_kind(conv)
    a, b = (gy, x) if transposed else (x, gy)          # a: the kernel's "input" operand, b: its "output gradient" operand
    N, Cin, H, W = a.shape
    Cout, Ho, Wo = b.shape[1], b.shape[2], b.shape[3]
    nbytes = ctypes.c_size_t(0)
    _native.call("octa_conv2d_f32_wgrad_workspace", N, Cin, H, W, Cout, K, s, pad, Ho, Wo, ctypes.byref(nbytes))
    ws = torch.empty(max(nbytes.value, 4), dtype=torch.uint8, device=x.device)
    dw = torch.empty((Cout, Cin, K, K), dtype=torch.float32, device=x.device)
    db = torch.empty((Cout,), dtype=torch.float32, device=x.device) if want_bias else None
    _native.launch("octa_conv2d_f32_wgrad_nchw", x.device, a, b, dw, db, ws, ws.numel(), N, Cin, H, W, Cout, K, s, pad, Ho, Wo)
    return dw, db


class ConvF32Train(torch.autograd.Function):
    """conv(x) with gradients, every product on the exact-fp32 kernels. dx is skipped when autograd does not need it (the first
    layer: the image records no gradient)."""

    @staticmethod
    def forward(ctx, x, weight, bias, conv):
        x = x.contiguous()
        ctx.conv = conv
        ctx.save_for_backward(x, weight)
        return forward(conv, x)

    @staticmethod
    def backward(ctx, gy):
        x, _ = ctx.saved_tensors
        conv = ctx.conv
        gy = gy.float().contiguous()
        dx = dgrad(conv, gy, x.shape) if ctx.needs_input_grad[0] else None
        dw = db = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw, db = wgrad(conv, x, gy, ctx.needs_input_grad[2])
            if not ctx.needs_input_grad[1]:
                dw = None
        return dx, dw, db, None


def train_forward(conv, x):
    """conv(x) for a layer `trainable` accepts, differentiable through ConvF32Train."""
    return ConvF32Train.apply(x, conv.weight, conv.bias, conv)
