"""Proves tests/_rotate_ref.py without a GPU. The float64 reference is torch's own F.affine_grid + F.grid_sample in float64 behind
torch.flip / torch.rot90, and the closed form on a linear ramp; two fp32 evaluations of the same operation stay inside the bounds on
every case that tests/test_rotate_gpu.py runs -- torch's fp32 grid_sample, and an emulation of the arithmetic of rotate_kernel in
csrc/augment.hip (g, sx, fx, floorf, the four weights, the tap permutation as index arithmetic); at angle 0 and N a power of two the
emulation is exactly the permuted input; and each of a list of wrong kernels (mutants of the emulation) breaks a bound or the exact check.
This is the evidence that the GPU tests can pass for a right kernel and fail for a wrong one. Flip of both axes commutes with rot90, so
"flip behind rot90" is the same operation and no mutant."""
import functools

import pytest
import torch
import torch.nn.functional as F

import _rotate_ref as R


def emulate(x, angle, rot_k=None, flip=None, threshold=None, mut=None):
    """rotate_kernel's own sequence in fp32, one rounding per torch operation"""
    B, N, _ = x.shape
    f32 = torch.float32
    Nf = torch.full((), float(N), dtype=f32)
    X, Y = torch.arange(N, dtype=f32)[None, None, :], torch.arange(N, dtype=f32)[None, :, None]
    c, s = torch.cos(angle.to(f32))[:, None, None], torch.sin(angle.to(f32))[:, None, None]
    if mut == "rotation_sign":
        s = -s
    if mut == "align_corners":              # affine_grid's base grid with align_corners = True, unnormalised as before
        d = torch.full((), float(max(N - 1, 1)), dtype=f32)
        gx, gy = 2.0 * X / d - 1.0, 2.0 * Y / d - 1.0
    elif mut == "no_half_pixel":
        gx, gy = 2.0 * X / Nf - 1.0, 2.0 * Y / Nf - 1.0
    else:
        gx, gy = (2.0 * X + 1.0) / Nf - 1.0, (2.0 * Y + 1.0) / Nf - 1.0
    sx, sy = c * gx - s * gy, s * gx + c * gy
    fx, fy = ((sx + 1.0) * Nf - 1.0) * 0.5, ((sy + 1.0) * Nf - 1.0) * 0.5
    x0f, y0f = (torch.trunc(fx), torch.trunc(fy)) if mut == "truncation" else (torch.floor(fx), torch.floor(fy))
    x0, y0 = x0f.long(), y0f.long()
    tx, ty = fx - x0f, fy - y0f
    k = (rot_k.long() if rot_k is not None else torch.zeros(B, dtype=torch.long))[:, None, None]
    fl = (flip.long() if flip is not None else torch.zeros(B, dtype=torch.long))[:, None, None] != 0
    if mut == "rot90_direction":
        k = (4 - k) % 4
    flat = x.to(f32).reshape(B, N * N)

    def tap(iy, ix):
        if mut == "border_clamp":
            iy, ix = iy.clamp(0, N - 1), ix.clamp(0, N - 1)
        ok = (iy >= 0) & (iy < N) & (ix >= 0) & (ix < N)
        iy, ix = iy.clamp(0, N - 1), ix.clamp(0, N - 1)
        y = torch.where(k == 1, ix, torch.where(k == 2, N - 1 - iy, torch.where(k == 3, N - 1 - ix, iy)))
        xx = torch.where(k == 1, N - 1 - iy, torch.where(k == 2, N - 1 - ix, torch.where(k == 3, iy, ix)))
        y = torch.where(fl, N - 1 - y, y)
        if mut != "flip_one_axis":
            xx = torch.where(fl, N - 1 - xx, xx)
        return torch.gather(flat, 1, (y * N + xx).reshape(B, -1)).reshape(iy.shape) * ok

    nw, ne, sw, se = (1.0 - tx) * (1.0 - ty), tx * (1.0 - ty), (1.0 - tx) * ty, tx * ty
    v = tap(y0, x0) * nw
    v = v + tap(y0, x0 + 1) * ne
    v = v + tap(y0 + 1, x0) * sw
    v = v + tap(y0 + 1, x0 + 1) * se
    if threshold is not None:
        v = ((v > threshold) if mut == "threshold_gt" else (v >= threshold)).to(f32)
    return v


def torch_grid_sample(x, angle, rot_k, flip, dtype):
    """F.affine_grid + F.grid_sample behind torch.flip / torch.rot90, in `dtype`, the angle's cosine and sine taken in `dtype` too"""
    B, N, _ = x.shape
    y = R.permute(x.to(dtype), rot_k, flip)
    a = angle.to(dtype)
    c, s, z = torch.cos(a), torch.sin(a), torch.zeros(B, dtype=dtype)
    theta = torch.stack([torch.stack([c, -s, z], 1), torch.stack([s, c, z], 1)], 1)
    grid = F.affine_grid(theta, (B, 1, N, N), align_corners=False)
    return F.grid_sample(y[:, None], grid, mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0]


@functools.lru_cache(maxsize=None)
def _prepared(N):
    return [(name, kind, x, angle, k, f) + R.reference(x, angle, k, f) for name, kind, x, angle, k, f in R.cases(N)]


@pytest.mark.parametrize("N", R.SIZES)
def test_reference_is_torch_grid_sample_in_float64(N):
    worst = 0.0
    for name, kind, x, angle, k, f, ref, tol in _prepared(N):
        want = torch_grid_sample(x, angle, k, f, torch.float64)
        worst = max(worst, float((ref - want).abs().max() / x.double().abs().max()))
    print("REFERENCE", N, "largest |ref - torch float64| / max |x|", worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("N", R.SIZES)
def test_reference_of_a_ramp_is_the_ramp_at_the_source_coordinates(N):
    """a flipped / turned ramp is a ramp p + q x + r y: where all four taps lie inside, the reference is p + q fx + r fy"""
    checked = 0
    for name, kind, x, angle, k, f, ref, tol in _prepared(N):
        if kind != "ramp":
            continue
        y = R.permute(x.double(), k, f)
        fx, fy = R.coords(N, angle, "cpu")
        p = y[:, 0, 0]
        q = y[:, 0, 1] - p if N > 1 else torch.zeros_like(p)
        r = y[:, 1, 0] - p if N > 1 else torch.zeros_like(p)
        want = p[:, None, None] + q[:, None, None] * fx + r[:, None, None] * fy
        inside = (fx >= 0) & (fx <= N - 1) & (fy >= 0) & (fy <= N - 1)
        assert float(((ref - want).abs() * inside).max()) <= 1e-12 * float(x.abs().max())
        checked += int(inside.sum())
    assert checked >= N * N


@pytest.mark.parametrize("N", R.SIZES)
def test_threshold_caps_hold_on_the_reference_alone(N):
    for name, kind, x, angle, k, f, ref, tol in _prepared(N):
        if kind in R.THRESHOLD:
            print("CAPS", N, name, "undecided share, decided ones, decided zeros:", R.caps(ref, tol, R.THRESHOLD[kind]))


@pytest.mark.parametrize("name", list(R.WINDOW_CASES))
def test_window_caps_hold_on_the_reference_alone(name):
    x, angle, k, f = R.window_case(name)
    N, size, offs = R.WINDOW_CASES[name]
    ref, tol = R.reference(x, angle, k, f, win=(size, offs))
    assert ref.shape == (3,) + size
    for thr in (0.1, 0.0):
        print("CAPS window", name, thr, R.caps(ref, tol, thr, classes=False))
    if name == "pad":           # the frame of zeros around the 37 x 37 image is exact and, at threshold 0, decided
        rim = torch.ones(48, 48, dtype=torch.bool)
        rim[5:42, 5:42] = False
        assert bool((ref[:, rim] == 0).all()) and bool((tol[:, rim] == 0).all()) and bool(R.decided(ref, tol, 0.0)[:, rim].all())
    # the emulation's window is the slice of its full frame by construction; it stays inside the window's bound
    got = R.window(emulate(x, angle, k, f), size, offs)
    assert R.ratio(got, ref, tol) <= 1.0
    for thr in (0.1, 0.0):
        got = R.window(emulate(x, angle, k, f), size, offs)
        assert R.discrete((got >= thr).float(), ref, tol, thr) == (0, 0)


@pytest.mark.parametrize("N", R.SIZES)
def test_fp32_evaluations_are_within_the_bounds(N):
    rat = {}
    for name, kind, x, angle, k, f, ref, tol in _prepared(N):
        rat[name + " torch"] = R.ratio(torch_grid_sample(x, angle, k, f, torch.float32), ref, tol)
        rat[name + " emulated"] = R.ratio(emulate(x, angle, k, f), ref, tol)
        if kind in R.THRESHOLD:
            thr = R.THRESHOLD[kind]
            assert R.discrete(emulate(x, angle, k, f, thr), ref, tol, thr) == (0, 0), (N, name)
            assert R.discrete((torch_grid_sample(x, angle, k, f, torch.float32) >= thr).float(), ref, tol, thr) == (0, 0), (N, name)
        if kind == "ones":          # the interior (further than the coordinate error from the rim) stays 1 within the value term alone
            fx, fy = R.coords(N, angle, "cpu")
            ds = R.coord_error(N)
            inside = (fx >= ds) & (fx <= N - 1 - ds) & (fy >= ds) & (fy <= N - 1 - ds)
            assert float(((emulate(x, angle, k, f).double() - 1.0).abs() * inside).max()) <= R.C_VAL * R.U
            if N >= 31:             # and the corners fade to 0: at 45 degrees they read nothing, whatever the roundings
                turned = angle == R.ANGLES[3]
                corners = lambda t: t[turned][:, [0, 0, -1, -1], [0, -1, 0, -1]]
                assert bool((corners(ref) == 0).all()) and bool((corners(tol) == 0).all()) and bool((corners(emulate(x, angle, k, f)) == 0).all())
    print("RATIO", N, {k_: float(f"{v:.3g}") for k_, v in rat.items()})
    print("RATIO max", N, "torch", max(v for k_, v in rat.items() if k_.endswith("torch")), "emulated", max(v for k_, v in rat.items() if k_.endswith("emulated")))
    assert all(v <= 1.0 for v in rat.values()), rat


def _pairs():
    return torch.arange(8, dtype=torch.int32) // 2, torch.arange(8, dtype=torch.int32) % 2


@pytest.mark.parametrize("N", [1, 2, 32, 256])
def test_emulation_at_angle_zero_is_exactly_the_permutation(N):
    """every coordinate is an integer in fp32 when N is a power of two: weights 1, 0, 0, 0. With values on a grid of eighths the
    threshold 0.5 meets exact ties."""
    k, f = _pairs()
    g = torch.Generator().manual_seed(N)
    x = torch.randn(8, N, N, generator=g)
    x8 = torch.randint(0, 9, (8, N, N), generator=g).float() / 8.0
    zero = torch.zeros(8)
    assert torch.equal(emulate(x, zero, k, f), R.permute(x, k, f))
    assert torch.equal(emulate(x8, zero, k, f, 0.5), (R.permute(x8, k, f) >= 0.5).float())
    ref, tol = R.reference(x8, zero, k, f)
    assert torch.equal(ref, R.permute(x8, k, f).double())


MUTANTS = ("align_corners", "rotation_sign", "rot90_direction", "flip_one_axis", "truncation", "border_clamp", "no_half_pixel", "threshold_gt")


def _exact_check_fails(mut):
    k, f = _pairs()
    x8 = torch.randint(0, 9, (8, 32, 32), generator=torch.Generator().manual_seed(32)).float() / 8.0
    zero = torch.zeros(8)
    return not (torch.equal(emulate(x8, zero, k, f, mut=mut), R.permute(x8, k, f))
                and torch.equal(emulate(x8, zero, k, f, 0.5, mut=mut), (R.permute(x8, k, f) >= 0.5).float()))


@pytest.mark.parametrize("mut", MUTANTS)
def test_mutant_is_rejected(mut):
    caught = ["exact N=32"] if _exact_check_fails(mut) else []
    for N in R.SIZES:
        for name, kind, x, angle, k, f, ref, tol in _prepared(N):
            bad = not R.ratio(emulate(x, angle, k, f, mut=mut), ref, tol) <= 1.0
            if kind in R.THRESHOLD:
                bad = bad or R.discrete(emulate(x, angle, k, f, R.THRESHOLD[kind], mut=mut), ref, tol, R.THRESHOLD[kind]) != (0, 0)
            if bad:
                caught.append(f"{N} {name}")
    print("MUTANT", mut, "caught on", len(caught), "cases:", caught)
    assert caught, f"nothing notices the mutant {mut}"
    if mut == "threshold_gt":       # equal to >= wherever there is no exact tie: only the exact check can see it
        assert caught == ["exact N=32"]
