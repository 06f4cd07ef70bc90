"""The bilinear resize pair of csrc/augment.hip (octa_resize_bilinear, octa_resize_bilinear_bwd, and BilinearResize around them) against
the float64 reference and the derived bounds of tests/_resize_ref.py (proved on the CPU by tests/test_resize_ref.py), and the claim of
the kernels' header that forward and adjoint agree to the last bit of every weight. Every test prints its error / bound ratios before
it asserts them.

Largest error / bound measured on an MI355X, on the kernels of commit dea40af, which the commit that adds this file leaves as they are:
    forward 0.261 (uint8, 2 x 257 -> 3 x 600; fp32 0.216)      adjoint 0.201 (64 x 48 -> 3 x 5; impulse matrices 0.305)
    BilinearResize in bf16: forward 0.986, adjoint 0.972 (50 x 70 -> 125 x 91: the one rounding to bf16 is a bound that half an ulp reaches)
    forward and adjoint impulse matrices: 0 differing entries on every shape"""
import pytest
import torch

import _resize_ref as rr

pytestmark = pytest.mark.gpu

DEV = "cuda"
IDS = lambda s: "x".join(map(str, s))


def _report(what, rat):
    print("RATIO", what, {k: float(f"{v:.4g}") for k, v in rat.items()})
    bad = {k: v for k, v in rat.items() if not v <= 1.0}
    assert not bad, f"{what}: error / bound above 1 for {bad} (all: {rat})"


@pytest.mark.parametrize("shape", rr.SHAPES, ids=IDS)
def test_forward(hip_lib_built, shape):
    """from uint8 and from fp32, with and without the intensity map"""
    from octa_autosegmentation_amd.data import gpu_augment
    h, w, H, W, B = shape
    x, x8, _, mul, add = rr.case(shape, DEV)
    rat = {}
    for name, src in (("fp32", x), ("uint8", x8)):
        rat[name] = rr.ratio(gpu_augment.resize_bilinear(src, (H, W)), *rr.forward(src, H, W))
        rat[name + " mul add"] = rr.ratio(gpu_augment.resize_bilinear(src, (H, W), mul, add), *rr.forward(src, H, W, mul, add))
    _report(f"resize forward {shape}", rat)
    if (h, w) == (H, W):        # every weight is 0 or 1
        assert torch.equal(gpu_augment.resize_bilinear(x, (H, W)), x) and torch.equal(gpu_augment.resize_bilinear(x8, (H, W)), x8.float())


@pytest.mark.parametrize("shape", rr.SHAPES, ids=IDS)
def test_adjoint(hip_lib_built, shape):
    """through resize_bilinear_bwd, and both ways through BilinearResize in fp32 and bf16 (one more rounding, of rounded inputs)"""
    from octa_autosegmentation_amd.data import gpu_augment
    h, w, H, W, B = shape
    x, _, dy, _, _ = rr.case(shape, DEV)
    rat = {"bwd": rr.ratio(gpu_augment.resize_bilinear_bwd(dy, (h, w)), *rr.adjoint(dy, h, w))}
    if (h, w) == (H, W):
        assert torch.equal(gpu_augment.resize_bilinear_bwd(dy, (h, w)), dy)
    for dtype in (torch.float32, torch.bfloat16):
        bf16 = dtype == torch.bfloat16
        xs, dys = x.to(dtype), dy.to(dtype)
        xm = xs[:, None].clone().requires_grad_(True)
        y = gpu_augment.BilinearResize.apply(xm, (H, W))
        assert y.dtype == dtype and y.shape == (B, 1, H, W)
        y.backward(dys[:, None])
        assert xm.grad.dtype == dtype and xm.grad.shape == (B, 1, h, w)
        rat[f"autograd fwd {dtype}"] = rr.ratio(y.detach(), *rr.forward(xs.float(), H, W, bf16=bf16))
        rat[f"autograd bwd {dtype}"] = rr.ratio(xm.grad, *rr.adjoint(dys.float(), h, w, bf16=bf16))
    _report(f"resize adjoint {shape}", rat)


@pytest.mark.parametrize("shape", rr.ADJOINT_SHAPES, ids=IDS)
def test_forward_and_adjoint_are_transposes_bit_for_bit(hip_lib_built, shape):
    """The forward's response to the h * w unit impulses and the adjoint's to the H * W unit impulses: each entry is one product of two
    weights, so the two dense matrices are equal after a transpose, with no tolerance. A window of the adjoint that is off by one
    loses an entry here."""
    from octa_autosegmentation_amd.data import gpu_augment
    h, w, H, W = shape
    assert h * w < 65535 and H * W < 65535
    fwd = gpu_augment.resize_bilinear(torch.eye(h * w, device=DEV).view(h * w, h, w).contiguous(), (H, W)).reshape(h * w, H * W)
    adj = gpu_augment.resize_bilinear_bwd(torch.eye(H * W, device=DEV).view(H * W, H, W).contiguous(), (h, w)).reshape(H * W, h * w)
    print("IMPULSE", shape, "entries", int((fwd != 0).sum()), "differing", int((fwd != adj.t()).sum()))
    assert torch.equal(fwd, adj.t())
    # and the matrix is the reference's, entry by entry, within the bound for one impulse
    ref, tol = rr.adjoint(torch.eye(H * W, device=DEV).view(H * W, H, W), h, w)
    _report(f"impulse matrix {shape}", {"adjoint": rr.ratio(adj, ref.reshape(H * W, h * w), tol.reshape(H * W, h * w))})

