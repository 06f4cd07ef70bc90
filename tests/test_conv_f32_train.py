"""CPU: the weight layouts of the exact-fp32 gradient kernels (models/conv_f32.py, csrc/conv_f32.hip), checked in pure torch.

The data-gradient kernels are the forward kernel run on dy with re-packed weights (a 3x3 stride-2 layer as four output-parity
sub-products stored scattered); the weight-gradient kernel computes dW[co][ci][tap] = sum dy[co][p] x[ci][p S + tap - pad], a transposed
layer with x and dy swapped. Here those products are restated with torch.nn.functional on the CPU, in float64, and compared with
torch.autograd.grad of the forward layer for every layer kind DynUNet-S holds, on odd sizes too."""
import pytest
import torch
import torch.nn.functional as F

from octa_autosegmentation_amd.models import conv_f32, networks


def _kernel_product(inp, wp, K, S, pad, Ho, Wo):
    """What conv_f32_kernel computes: out[co](oy, ox) = sum_{ci, r, s} inp[ci](oy S + r - pad, ox S + s - pad) wp[ci][r K + s][co], reads
    outside the map are zero (also beyond the bottom / right edge, where a parity sub-product reads one row / column past dy)."""
    cin, cout = wp.shape[0], wp.shape[2]
    w = wp.reshape(cin, K, K, cout).permute(3, 0, 1, 2)
    x = F.pad(inp, (pad, K + S, pad, K + S))
    return F.conv2d(x, w, stride=S)[:, :, :Ho, :Wo]


def _dx_from_layout(conv, dy, x_shape):
    kind = conv_f32._layer_kind(conv)
    K, S, pad, transposed = kind
    wd = conv_f32.dgrad_layout(conv.weight.detach().double(), kind)
    N, Cin, H, W = x_shape
    if transposed:
        return _kernel_product(dy, wd, K, K, 0, H, W)
    if S == 1:
        return _kernel_product(dy, wd, K, 1, K - 1 - pad, H, W)
    assert wd.shape == (4, dy.shape[1], 4, Cin)
    dx = torch.full(x_shape, float("nan"), dtype=torch.float64)
    for a in range(2):
        for b in range(2):
            hp, wp = (H - a + 1) // 2, (W - b + 1) // 2
            blk = wd[2 * a + b]
            if (a, b) == (0, 0):                 # one tap: a 1x1 product on tap slot 0; the other three slots are zero
                assert torch.count_nonzero(blk[:, 1:, :]) == 0
                part = _kernel_product(dy, blk[:, :1, :], 1, 1, 0, hp, wp)
            else:
                part = _kernel_product(dy, blk, 2, 1, 0, hp, wp)
            dx[:, :, a::2, b::2] = part
    return dx


def _dw_product(x, dy, K, S, pad):
    """dW[co][ci][r][s] = sum_{n, p} dy[n][co][p] x[n][ci][p S + (r, s) - pad] (unfold form)."""
    N, Cin = x.shape[:2]
    Cout, Ho, Wo = dy.shape[1:]
    cols = F.unfold(F.pad(x, (pad, K + S, pad, K + S)), K, stride=S)     # [N][Cin K K][L]
    nx = (x.shape[3] + pad + S) // S + 1                                  # columns of the padded map
    cols = cols.reshape(N, Cin * K * K, -1, nx)[:, :, :Ho, :Wo].reshape(N, Cin * K * K, Ho * Wo)
    return torch.einsum("ncp,nkp->ck", dy.reshape(N, Cout, Ho * Wo), cols).reshape(Cout, Cin, K, K)


CASES = [  # (layer, input shape)
    (torch.nn.Conv2d(3, 5, 3, 1, 1, bias=False), (2, 3, 9, 11)),
    (torch.nn.Conv2d(1, 8, 3, 1, 1, bias=False), (1, 1, 7, 6)),
    (torch.nn.Conv2d(4, 6, 3, 2, 1, bias=False), (2, 4, 10, 12)),
    (torch.nn.Conv2d(4, 6, 3, 2, 1, bias=False), (1, 4, 11, 9)),          # odd sizes: the odd parities are one row / column shorter
    (torch.nn.Conv2d(3, 2, 3, 2, 1, bias=False), (1, 3, 1, 5)),           # one row: no odd rows at all
    (torch.nn.Conv2d(6, 1, 1, 1, 0, bias=True), (2, 6, 5, 7)),            # the output head
    (torch.nn.ConvTranspose2d(6, 4, 2, 2, bias=False), (2, 6, 5, 3)),
    (torch.nn.ConvTranspose2d(7, 3, 1, 1, bias=False), (1, 7, 4, 9)),
]


@pytest.mark.parametrize("mod,shape", CASES, ids=[f"{type(m).__name__}-k{m.kernel_size[0]}s{m.stride[0]}-{s}" for m, s in CASES])
def test_gradient_layouts_match_autograd(mod, shape):
    torch.manual_seed(0)
    mod = mod.double()
    x = torch.randn(*shape, dtype=torch.float64, requires_grad=True)
    y = mod(x)
    dy = torch.randn_like(y)
    params = [mod.weight] + ([mod.bias] if mod.bias is not None else [])
    grads = torch.autograd.grad(y, [x] + params, dy)
    dx = _dx_from_layout(mod, dy, x.shape)
    assert torch.allclose(dx, grads[0], rtol=1e-12, atol=1e-12), (dx - grads[0]).abs().max()
    K, S, pad, transposed = conv_f32._layer_kind(mod)
    dw = _dw_product(dy, x.detach(), K, S, 0) if transposed else _dw_product(x.detach(), dy, K, S, pad)
    assert dw.shape == mod.weight.shape
    assert torch.allclose(dw, grads[1], rtol=1e-12, atol=1e-12), (dw - grads[1]).abs().max()
    if mod.bias is not None:
        assert torch.allclose(dy.sum(dim=(0, 2, 3)), grads[2], rtol=1e-12, atol=1e-12)


def test_every_dynunet_layer_is_covered():
    net = networks.DynUNet(filters=[8, 16, 16, 16, 16])
    convs = [m for m in net.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d))]
    assert len(convs) >= 19
    kinds = {conv_f32._layer_kind(c) for c in convs}
    assert None not in kinds
    assert kinds == {(3, 1, 1, False), (3, 2, 1, False), (1, 1, 0, False), (2, 2, 0, True), (1, 1, 0, True)}


def test_uncovered_layers_are_refused():
    for m in (torch.nn.Conv2d(4, 4, 7, 1, 3), torch.nn.Conv2d(4, 4, 4, 1, 1), torch.nn.Conv2d(4, 4, 3, 1, 0),
              torch.nn.Conv2d(4, 4, 3, 1, 1, padding_mode="reflect"), torch.nn.Conv2d(4, 4, 3, 1, 1, groups=2),
              torch.nn.ConvTranspose2d(4, 4, 2, 2, bias=True), torch.nn.ConvTranspose2d(4, 4, 3, 2, 1)):
        assert conv_f32._layer_kind(m) is None, m
    # CPU tensors never take the GPU path
    assert not conv_f32.trainable(torch.nn.Conv2d(4, 4, 3, 1, 1), torch.randn(1, 4, 8, 8, requires_grad=True))


def test_dgrad_pack_is_cached_per_weight_version():
    conv = torch.nn.Conv2d(4, 6, 3, 2, 1, bias=False)
    kind = conv_f32._layer_kind(conv)
    p1 = conv_f32._packed_dgrad(conv.weight, kind)
    assert conv_f32._packed_dgrad(conv.weight, kind) is p1
    fwd = conv_f32._packed(conv.weight, False)                  # the forward pack lives under its own attribute
    assert conv_f32._packed_dgrad(conv.weight, kind) is p1 and conv_f32._packed(conv.weight, False) is fwd
    with torch.no_grad():
        conv.weight.mul_(2.0)                                    # an optimiser step: the version moves
    p2 = conv_f32._packed_dgrad(conv.weight, kind)
    assert p2 is not p1 and torch.equal(p2, 2.0 * p1)
