"""rotate_kernel and rotate_window_kernel of csrc/augment.hip (octa_flip_rot90_rotate, octa_flip_rot90_rotate_window) against the float64
reference and the derived bounds of tests/_rotate_ref.py (proved on the CPU by tests/test_rotate_ref.py): every shared case within its
bound, thresholded output exact on every decided pixel, angle 0 at a power-of-two size exactly the flip / rot90 of the input (ties of
the threshold included), the window form against the reference and no longer only against its sibling. Every output lies between
sentinels, every launch runs twice with equal bits, and every test prints its error / bound ratios before it asserts them.

Largest error / bound measured on an MI355X, on the kernels of commit c9efa0d, which the commit that adds this file leaves as they are:
    full frame 0.107 (N = 257, the constant image at 0.7854 / 3.0; N = 304: 0.101)      window 0.075 (300 -> 280 x 290)
    thresholded: 0 wrong decided pixels, 0 values other than 0 and 1 on every case; angle 0 at N = 32 and 256: 0 differing elements, with
    942 and 58803 exact ties of the threshold among them"""
import pytest
import torch

import _rotate_ref as R
from _guarded import Guarded

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _run(x, angle, k, f, thr=None, win=None):
    """The entry point itself, twice, into sentinel-guarded buffers -> the output; asserts equal bits and intact rims."""
    from octa_autosegmentation_amd import _native
    B, N = x.shape[0], x.shape[1]
    outs = []
    for _ in range(2):
        if win is None:
            g = Guarded((B, N, N), torch.float32)
            _native.launch("octa_flip_rot90_rotate", x.device, x, g.t, B, N, angle, k, f, float(thr if thr is not None else 0.0), 0 if thr is None else 1)
        else:
            size, oy, ox = win
            g = Guarded((B, size[0], size[1]), torch.float32)
            _native.launch("octa_flip_rot90_rotate_window", x.device, x, g.t, B, N, angle, k, f, float(thr if thr is not None else 0.0),
                           0 if thr is None else 1, size[0], size[1], oy, ox)
        torch.cuda.synchronize()
        assert g.intact() and g.unwritten() == 0
        outs.append(g.t.clone())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    return outs[0]


def _report(what, rat):
    print("RATIO", what, {k: float(f"{v:.4g}") for k, v in rat.items()})
    bad = {k: v for k, v in rat.items() if not v <= 1.0}
    assert not bad, f"{what}: error / bound above 1 for {bad}"


@pytest.mark.parametrize("N", R.SIZES)
def test_full_frame_kernel(hip_lib_built, N):
    from octa_autosegmentation_amd.data import gpu_augment
    rat = {}
    for name, kind, x, angle, k, f in R.cases(N):
        x, angle, k, f = R.to(DEV, x, angle, k, f)
        ref, tol = R.reference(x, angle, k, f)
        got = _run(x, angle, k, f)
        rat[name] = R.ratio(got, ref, tol)
        assert torch.equal(gpu_augment.flip_rot90_rotate(x, angle, k, f), got)
        if kind in R.THRESHOLD:
            thr = R.THRESHOLD[kind]
            caps = R.caps(ref, tol, thr)
            wrong, other = R.discrete(_run(x, angle, k, f, thr), ref, tol, thr)
            print("DISCRETE", N, name, "threshold", thr, "undecided share / decided ones / zeros", caps, "wrong", wrong, "not 0 or 1", other)
            assert wrong == 0 and other == 0, (N, name)
    _report(f"rotate {N}", rat)


@pytest.mark.parametrize("N", [32, 256])
def test_angle_zero_is_exactly_the_flip_and_rot90(hip_lib_built, N):
    """no tolerance: every coordinate is an integer in fp32, the weights are 1, 0, 0, 0; values on a grid of eighths meet the threshold 0.5"""
    k, f = torch.arange(8, dtype=torch.int32, device=DEV) // 2, torch.arange(8, dtype=torch.int32, device=DEV) % 2
    g = torch.Generator().manual_seed(N)
    x = torch.randn(8, N, N, generator=g).to(DEV)
    x8 = (torch.randint(0, 9, (8, N, N), generator=g).float() / 8.0).to(DEV)
    zero = torch.zeros(8, device=DEV)
    want, want8 = R.permute(x, k, f), R.permute(x8, k, f)
    got, got8 = _run(x, zero, k, f), _run(x8, zero, k, f, 0.5)
    print("EXACT", N, "differing", int((got != want).sum()), "differing after the threshold", int((got8 != (want8 >= 0.5).float()).sum()),
          "ties", int((want8 == 0.5).sum()))
    assert int((want8 == 0.5).sum()) > N
    assert torch.equal(got, want)
    assert torch.equal(got8, (want8 >= 0.5).float())


@pytest.mark.parametrize("name", list(R.WINDOW_CASES))
def test_window_kernel_against_the_reference(hip_lib_built, name):
    """the window is the slice of the zero-extended reference; the padding is exactly 0 and goes through the threshold (at 0 it becomes 1)"""
    N, size, offs = R.WINDOW_CASES[name]
    x, angle, k, f = R.to(DEV, *R.window_case(name))
    oy = torch.tensor([o[0] for o in offs], dtype=torch.int32, device=DEV)
    ox = torch.tensor([o[1] for o in offs], dtype=torch.int32, device=DEV)
    ref, tol = R.reference(x, angle, k, f, win=(size, offs))
    rat = {}
    for thr in R.WINDOW_THRESHOLDS:
        got = _run(x, angle, k, f, thr, (size, oy, ox))
        if thr is None:
            rat["window"] = R.ratio(got, ref, tol)
        else:
            caps = R.caps(ref, tol, thr, classes=False)
            wrong, other = R.discrete(got, ref, tol, thr)
            print("DISCRETE window", name, "threshold", thr, "undecided share / decided ones / zeros", caps, "wrong", wrong, "not 0 or 1", other)
            assert wrong == 0 and other == 0, (name, thr)
        if name == "pad":
            assert bool((got[:, :5] == (1.0 if thr == 0.0 else 0.0)).all()) and bool((got[:, :, 42:] == (1.0 if thr == 0.0 else 0.0)).all())
    _report(f"rotate window {name}", rat)


def test_full_frame_entry_point_refuses_bad_arguments(hip_lib_built):
    """An error code and a message, not a launch: the output keeps its sentinel."""
    from octa_autosegmentation_amd import _native
    dev = torch.device(DEV)
    x = torch.rand((2, 16, 16), device=dev)
    out = Guarded((2, 16, 16), torch.float32)
    ang = torch.zeros(2, device=dev)
    lib, ctx, stream = _native.lib(), _native.ctx(dev.index), _native.current_stream_ptr()
    good = [x.data_ptr(), out.t.data_ptr(), 2, 16, ang.data_ptr(), None, None, 0.0, 0]

    def bad(i, v):
        a = list(good)
        a[i] = v
        return a

    for args in (bad(1, x.data_ptr()), bad(2, 0), bad(2, 65536), bad(3, 0), bad(3, 65536), bad(0, None), bad(1, None), bad(4, None)):
        assert lib.octa_flip_rot90_rotate(ctx, *args, stream) == -2
        assert lib.octa_last_error().decode() == "octa_flip_rot90_rotate: bad arguments"
    assert lib.octa_flip_rot90_rotate(None, *good, stream) == -2
    with pytest.raises(_native.OctaHipError):
        _native.launch("octa_flip_rot90_rotate", dev, x, out.t, 2, 0, ang, None, None, 0.0, 0)
    torch.cuda.synchronize()
    assert out.untouched()
    assert lib.octa_flip_rot90_rotate(ctx, *good, stream) == 0
    torch.cuda.synchronize()
    assert out.intact() and torch.equal(out.t, x)            # angle 0, no flip, no turn, N a power of two: the input itself
