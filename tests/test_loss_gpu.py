"""The fused Dice + BCE kernels of csrc/loss.hip and their dispatch in models/losses.py against the float64 reference and the derived
bounds of tests/_loss_ref.py (proved on the CPU by tests/test_loss_ref.py). Every test prints its error / bound ratios before it asserts
them.

Largest error / bound measured on an MI355X (256 CUs), on the kernels of commit dea40af, which the commit that adds this file leaves as
they are:
    sums 0.153 (case 6-empty-30, fp32)      loss 0.332 (case 6-empty-15, fp32)
    dx fp32 0.610 (autograd, (2, 3, 17, 19); entry points 0.571, case 8-bwd-cap)
    dx bf16 0.996 (case 8-fwd-cap: the one rounding to bf16 is a bound that half an ulp reaches)
    dispatch: loss 0.047, dx 0.414"""
import pytest
import torch

import _loss_ref as lr

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 7.5          # exact in bf16
GUARD = 1024


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _report(what, rat):
    print("RATIO", what, {k: float(f"{v:.4g}") for k, v in rat.items()})
    lr.assert_within(rat, what)


def _entry(x, t, g):
    """the three entry points on the calling thread, with buffers of the test's own -> sums, loss, dx"""
    from octa_autosegmentation_amd import _native
    rows, n = x.shape
    dt = 0 if x.dtype == torch.float32 else 1
    sums = torch.full((rows, 4), -3.0e30, dtype=torch.float64, device=DEV)           # the forward has to clear it
    _native.launch("octa_dice_bce_fwd", x.device, x, dt, t, rows, n, sums)
    loss = torch.full((), float("nan"), dtype=torch.float32, device=DEV)
    _native.launch("octa_dice_bce_finish", x.device, sums, rows, n, lr.NR, lr.DR, loss)
    buf = torch.full((rows * n + GUARD,), float("nan"), dtype=x.dtype, device=DEV)     # an element the backward leaves out stays NaN
    buf[rows * n:] = SENTINEL
    gout = torch.tensor([g], dtype=torch.float32, device=DEV)
    _native.launch("octa_dice_bce_bwd", x.device, x, dt, t, rows, n, sums, gout, lr.NR, lr.DR, buf)
    torch.cuda.synchronize()
    assert (buf[rows * n:] == SENTINEL).all(), "the backward wrote past rows * n"
    return dict(sums=sums, loss=loss, dx=buf[:rows * n].view(rows, n))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cid", list(lr.CASES))
def test_entry_points(hip_lib_built, cid, dtype):
    bf16 = dtype == torch.bfloat16
    cus = _cus()
    x, t, g = lr.case(cid, cus=cus, device=DEV, bf16=bf16)
    assert x.dtype == dtype and x.is_contiguous() and t.is_contiguous()
    rows, n = x.shape
    r = lr.reference(x, t, g)                   # of the rounded logits where they are bf16
    tol = lr.bounds(r, lr.trips(n, rows, cus, "fwd"), bf16=bf16)
    got = _entry(x, t, g)
    print("GRID", cid, "rows", rows, "n", n, "fwd gx", lr.grid_x(n, rows, cus, "fwd"), "trips", lr.trips(n, rows, cus, "fwd"),
          "bwd gx", lr.grid_x(n, rows, cus, "bwd"), "trips", lr.trips(n, rows, cus, "bwd"))
    _report(f"entry {cid} {'bf16' if bf16 else 'fp32'}", lr.ratios(r, tol, got))


def _inputs(shape, seed, dtype):
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(shape, generator=gen) * 3.0).to(dtype).to(DEV)
    t = (torch.rand(shape, generator=gen) > 0.8).float().to(DEV)
    return x, t


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 1, 17, 19), (2, 3, 17, 19), (1, 44, 8, 8), (2, 1, 3, 4, 5)], ids=lambda s: "x".join(map(str, s)))
def test_autograd(hip_lib_built, shape, dtype):
    """DiceBCELoss(True) as the trainers call it, with an upstream gradient that is not 1"""
    from octa_autosegmentation_amd.models import losses
    assert losses.USE_FUSED_LOSS
    x, t = _inputs(shape, 4000 + sum(shape), dtype)
    xm = x.clone().requires_grad_(True)
    loss = losses.DiceBCELoss(True)(xm, t)
    assert loss.dtype == torch.float32 and loss.shape == ()
    (loss * 0.37).backward()
    assert xm.grad.dtype == dtype and xm.grad.shape == x.shape
    rows = shape[0] * shape[1]
    r = lr.reference(x.reshape(rows, -1), t.reshape(rows, -1), lr.f32(0.37))
    tol = lr.bounds(r, lr.trips(r.n, rows, _cus(), "fwd"), bf16=dtype == torch.bfloat16)
    _report(f"autograd {shape} {dtype}", lr.ratios(r, tol, dict(loss=loss.detach(), dx=xm.grad.reshape(rows, -1))))


# shape -> (rows, n) of the composition's reduction, and whether the kernels take the call
DISPATCH = [((6,), (1, 6), False), ((6, 1), (1, 6), False), ((4, 1, 5), (4, 5), True), ((4, 1, 3, 5), (4, 15), True), ((2, 3, 4, 5), (6, 20), True),
            ((8192, 8, 1, 2), (65536, 2), False), ((65536, 1, 1, 3), (65536, 3), False)]


@pytest.mark.parametrize("shape,view,fused", DISPATCH, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_dispatch_gives_the_composition(hip_lib_built, shape, view, fused, monkeypatch):
    """With USE_FUSED_LOSS on, every shape gets the value of (Dice(sigmoid) + BCEWithLogits) / 2: within the kernels' bounds where they
    take the call, and within what an fp32 composition may lose where they do not. Without spatial dimensions the composition's Dice
    reduces over everything, which is one row of all elements in the terms of the reference."""
    from octa_autosegmentation_amd.models import losses
    assert losses.USE_FUSED_LOSS
    x, t = _inputs(shape, 4100 + len(shape) + shape[0], torch.float32)
    calls = []
    real = losses._FusedDiceBCE.apply
    monkeypatch.setattr(losses._FusedDiceBCE, "apply", lambda *a: (calls.append(1), real(*a))[1])
    xm = x.clone().requires_grad_(True)
    loss = losses.DiceBCELoss(True)(xm, t)
    (loss * 0.37).backward()
    assert bool(calls) == fused
    # the composition itself in float64 (not a CUDA tensor: no dispatch), and the hand-written reference in the composition's row structure
    xc = x.double().cpu().requires_grad_(True)
    want = losses.DiceBCELoss(True)(xc, t.double().cpu())
    (want * lr.f32(0.37)).backward()
    r = lr.reference(x.reshape(view), t.reshape(view), lr.f32(0.37))
    assert abs(want.item() - r.loss.item()) <= 1e-12 and torch.allclose(xc.grad.reshape(view).to(DEV), r.dx, rtol=1e-9, atol=1e-15)
    rows, n = view
    if fused:
        tol = lr.bounds(r, lr.trips(n, rows, _cus(), "fwd"))
    else:
        # torch in fp32: a row's sums chain at most n additions, the two means at most rows * n (the worst any fp32 summation order does)
        tol = lr.bounds(r, n)
        tol.loss = tol.loss + rows * n * lr.U * ((1.0 - r.N / r.D).abs().mean() + r.sums[:, 3].sum() / (rows * n)) / 2.0
    _report(f"dispatch {shape}", lr.ratios(r, tol, dict(loss=loss.detach(), dx=xm.grad.reshape(view))))

