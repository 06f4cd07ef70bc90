"""Proves tests/_resize_ref.py without a GPU. Two fp32 evaluations of the bilinear resize stay inside the bounds on every shape that
tests/test_resize_gpu.py runs -- torch's own F.interpolate with its autograd, and an emulation of the arithmetic of csrc/augment.hip
(fp32 source index, truncation, 1 - lambda, the two-by-two combination; the adjoint as a sum of weight products) -- and each of a list of
wrong kernels (mutants of the emulation) breaks a bound. This is the evidence that the GPU tests can pass for a right kernel and fail
for a wrong one."""
import functools

import pytest
import torch
import torch.nn.functional as F

import _resize_ref as rr


def _axis32(n_src, n_dst, mut=None, ratio=None):
    """the kernel's per-axis quantities in fp32 -> i1, step to the second tap (0 / 1), l0, l1"""
    one = torch.ones((), dtype=torch.float32)
    d = torch.arange(n_dst, dtype=torch.float32)
    if mut == "align_corners":
        s = (one * (n_src - 1) / max(n_dst - 1, 1)) * d
    else:
        s = (one * n_src / n_dst if ratio is None else ratio) * (d + 0.5) - 0.5
        if mut != "no_clamp":
            s = s.clamp_min(0)
    i1 = s.to(torch.int64).clamp_max(n_src - 1)        # (int) truncates towards zero
    p = (i1 < n_src - 1).long()
    l1 = s - i1.float()
    return i1, p, 1.0 - l1, l1


def emulate_forward(x, H, W, mul=None, add=None, mut=None):
    B, h, w = x.shape
    one = torch.ones((), dtype=torch.float32)
    v = x.float()
    if mut != "affine_after":
        v = v * (mul[:, None, None] if mul is not None else 1.0) + (add[:, None, None] if add is not None else 0.0)
    ry, rx = (one * w / W, one * h / H) if mut == "swapped_ratio" else (None, None)
    iy, py, hy0, hy1 = _axis32(h, H, mut, ry)
    ix, px, wx0, wx1 = _axis32(w, W, mut, rx)
    top, bot = v[:, iy], v[:, iy + py]
    hy0, hy1 = hy0[None, :, None], hy1[None, :, None]
    out = hy0 * (wx0 * top[:, :, ix] + wx1 * top[:, :, ix + px]) + hy1 * (wx0 * bot[:, :, ix] + wx1 * bot[:, :, ix + px])
    if mut == "affine_after":
        out = out * mul[:, None, None] + add[:, None, None]
    return out


def _weights32(n_src, n_dst, mut=None, ratio=None, short=None):
    """tap_weight as a matrix [src][dst]; short = "first" / "last": the window of every source index misses its first / last output"""
    i1, p, l0, l1 = _axis32(n_src, n_dst, mut, ratio)
    src = torch.arange(n_src)[:, None]
    Wt = torch.where(i1[None] == src, l0[None], torch.zeros(())) + torch.where((i1 + p)[None] == src, l1[None], torch.zeros(()))
    if short:
        for s in range(n_src):
            nz = Wt[s].nonzero().flatten()
            if len(nz):
                Wt[s, nz[0] if short == "first" else nz[-1]] = 0.0
    return Wt


def emulate_adjoint(dy, h, w, mut=None):
    B, H, W = dy.shape
    one = torch.ones((), dtype=torch.float32)
    ry, rx = (one * w / W, one * h / H) if mut == "swapped_ratio" else (None, None)
    Wy = _weights32(h, H, mut, ry)
    Wx = _weights32(w, W, mut, rx, short={"window_short_left": "first", "window_short_right": "last"}.get(mut))
    row = torch.einsum("bYX,xX->bYx", dy.float(), Wx)       # row += wx * g
    return torch.einsum("yY,bYx->byx", Wy, row)             # acc += wy * row


@functools.lru_cache(maxsize=None)
def _prepared(shape):
    h, w, H, W, B = shape
    x, x8, dy, mul, add = rr.case(shape)
    return x, x8, dy, mul, add, rr.forward(x, H, W), rr.forward(x, H, W, mul, add), rr.forward(x8, H, W, mul, add), rr.adjoint(dy, h, w)


@pytest.mark.parametrize("shape", rr.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fp32_evaluations_are_within_the_bounds(shape):
    h, w, H, W, B = shape
    x, x8, dy, mul, add, plain, affine, affine8, adj = _prepared(shape)
    xt = x[:, None].clone().requires_grad_(True)
    yt = F.interpolate(xt, size=(H, W), mode="bilinear", align_corners=False)
    yt.backward(dy[:, None])
    rat = {
        "torch fwd": rr.ratio(yt.detach(), *plain),
        "torch fwd affine": rr.ratio(F.interpolate((x * mul[:, None, None] + add[:, None, None])[:, None], size=(H, W), mode="bilinear", align_corners=False), *affine),
        "torch adjoint": rr.ratio(xt.grad, *adj),
        "emulated fwd": rr.ratio(emulate_forward(x, H, W), *plain),
        "emulated fwd affine": rr.ratio(emulate_forward(x, H, W, mul, add), *affine),
        "emulated fwd uint8": rr.ratio(emulate_forward(x8, H, W, mul, add), *affine8),
        # weights sum to one: the affine map may as well come last. Identical in exact arithmetic, so the bound must not notice
        "emulated fwd, affine map last": rr.ratio(emulate_forward(x, H, W, mul, add, mut="affine_after"), *affine),
        "emulated adjoint": rr.ratio(emulate_adjoint(dy, h, w), *adj),
    }
    print(shape, {k: float(f"{v:.3g}") for k, v in rat.items()})
    assert all(v <= 1.0 for v in rat.values()), rat
    if (h, w) == (H, W):
        assert torch.equal(emulate_forward(x, H, W), x) and torch.equal(emulate_adjoint(dy, h, w), dy)      # every weight is 0 or 1


def test_reference_adjoint_is_the_transpose_of_the_reference_forward():
    for shape in rr.SHAPES[:-1]:
        h, w, H, W, B = shape
        x, _, dy, _, _, plain, _, _, adj = _prepared(shape)
        lhs, rhs = (plain[0] * dy.double()).sum().item(), (x.double() * adj[0]).sum().item()
        assert abs(lhs - rhs) <= 1e-12 * (plain[0] * dy.double()).abs().sum().item(), shape


FORWARD_MUTANTS = ("align_corners", "no_clamp", "swapped_ratio")
ADJOINT_MUTANTS = ("align_corners", "no_clamp", "swapped_ratio", "window_short_left", "window_short_right")


@pytest.mark.parametrize("mut", FORWARD_MUTANTS)
def test_forward_mutant_is_rejected(mut):
    caught = []
    for shape in rr.SHAPES[:-1]:
        h, w, H, W, B = shape
        x, _, _, mul, add, _, affine, _, _ = _prepared(shape)
        if not rr.ratio(emulate_forward(x, H, W, mul, add, mut=mut), *affine) <= 1.0:
            caught.append(shape)
    print(mut, "caught on", caught)
    assert caught, f"no bound notices the forward mutant {mut}"


@pytest.mark.parametrize("mut", ADJOINT_MUTANTS)
def test_adjoint_mutant_is_rejected(mut):
    caught = []
    for shape in rr.SHAPES[:-1]:
        h, w, H, W, B = shape
        dy, adj = _prepared(shape)[2], _prepared(shape)[8]
        if not rr.ratio(emulate_adjoint(dy, h, w, mut=mut), *adj) <= 1.0:
            caught.append(shape)
    print(mut, "caught on", caught)
    assert caught, f"no bound notices the adjoint mutant {mut}"
    if mut.startswith("window"):        # a window that is short misses something wherever an index has an output at all
        assert len(caught) >= len(rr.SHAPES) - 2, caught


def test_impulse_matrices_of_the_emulation_are_transposes():
    """what tests/test_resize_gpu.py asks of the kernels bit for bit: the forward's response to the unit impulses is the adjoint's,
    transposed (without contraction every entry is one product of two weights, rounded once)"""
    for (h, w, H, W) in rr.ADJOINT_SHAPES:
        fwd = emulate_forward(torch.eye(h * w).view(h * w, h, w), H, W).reshape(h * w, H * W)
        adj = emulate_adjoint(torch.eye(H * W).view(H * W, H, W), h, w).reshape(H * W, h * w)
        assert torch.equal(fwd, adj.t()), (h, w, H, W)
