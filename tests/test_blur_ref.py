"""Proves tests/_blur_ref.py without a GPU. The float64 references agree with the torch expressions tests/test_blur_gpu.py compares with
(reflect / replicate pad and grouped (transposed) convolution, in float64, to 1e-12) and with float64 autograd of them for the three
backward operations. An fp32 emulation of each kernel of csrc/blur.hip -- its tap generators refl, pad_sources, down_taps and up_taps
written out again index by index, its sums in the kernel's order, one round-to-nearest-even on a bf16 store, reads by flat address from
a buffer that ends in NaNs -- gives the one legal result on the exact cases, the reference's impulse matrices bit for bit, and stays inside
every bound on the real-valued cases. Each of a list of wrong kernels (mutants of the emulation) breaks a bound, an exact case or an impulse
matrix. This is the evidence that the GPU tests can pass for a right kernel and fail for a wrong one."""
import functools

import pytest
import torch
import torch.nn.functional as F

import _blur_ref as br

NAN = float("nan")


# ---- the torch expressions of tests/test_blur_gpu.py, in float64 ---------------------------------------------------------------------------

def _torch_op(kind, x, pad):
    c = x.shape[1]
    if kind == "pad":
        return F.pad(x, [pad] * 4, mode="reflect")
    if kind == "down":
        a = torch.tensor([1., 2., 1.], dtype=x.dtype)
        f = (a[:, None] * a[None, :] / 16)[None, None].repeat(c, 1, 1, 1)
        return F.conv2d(F.pad(x, [1, 1, 1, 1], mode="reflect"), f, stride=2, groups=c)
    a = torch.tensor([1., 3., 3., 1.], dtype=x.dtype)
    f = (a[:, None] * a[None, :] / 64 * 4)[None, None].repeat(c, 1, 1, 1)
    y = F.conv_transpose2d(F.pad(x, [1, 1, 1, 1], mode="replicate"), f, stride=2, padding=2, groups=c)
    return y[:, :, 1:, 1:][:, :, :-1, :-1]


@pytest.mark.parametrize("kind", ["pad", "down", "up"])
def test_references_agree_with_the_torch_expressions_and_their_autograd(kind):
    shapes = [(s, br.PADS[s]) for s in br.SHAPES] + [((1, 2, h, w), min(h, w) - 1) for h, w in br.IMPULSE_HW]
    if kind == "up":
        shapes += [((1, 2, h, w), 0) for h, w in br.IMPULSE_UP_EXTRA]
    for (B, C, H, W), pad in shapes:
        gen = torch.Generator().manual_seed(H * 31 + W)
        x = torch.randn((B, C, H, W), generator=gen, dtype=torch.float64).requires_grad_(True)
        y = _torch_op(kind, x, pad)
        g = torch.randn(y.shape, generator=gen, dtype=torch.float64)
        y.backward(g)
        ref, _ = br.reference(kind + "_fwd", x.detach().permute(0, 2, 3, 1), H, W, pad)
        dref, _ = br.reference(kind + "_bwd", g.permute(0, 2, 3, 1), H, W, pad)
        assert ref.shape[1:3] == br.out_hw(kind + "_fwd", H, W, pad)
        assert (ref.permute(0, 3, 1, 2) - y.detach()).abs().max().item() <= 1e-12, (kind, H, W, pad)
        assert (dref.permute(0, 3, 1, 2) - x.grad).abs().max().item() <= 1e-12, (kind, H, W, pad)


def test_weights_of_the_operators():
    """forward rows sum to 1, transposed rows of the blurs to at most 4 (64/16), every entry a multiple of 1/16 after the second axis"""
    for n in range(1, 12):
        up = br.axis("up", n)
        assert torch.equal(up.sum(1), torch.ones(2 * n, dtype=torch.float64)) and up.sum(0).max().item() <= 2.0
        if n >= 2:
            dn = br.axis("down", n)
            assert torch.equal(dn.sum(1), torch.ones(dn.shape[0], dtype=torch.float64)) and dn.sum(0).max().item() <= 2.0
            for pad in range(1, n):
                pd = br.axis("pad", n, pad)
                assert torch.equal(pd.sum(1), torch.ones(n + 2 * pad, dtype=torch.float64)) and pd.sum(0).max().item() <= 3.0


# ---- the emulation -------------------------------------------------------------------------------------------------------------------------

def _refl(p, n, mut):
    if mut == "refl_repeat":                       # a reflection that repeats the border
        return -p - 1 if p < 0 else (2 * n - 1 - p if p >= n else p)
    return -p if p < 0 else (2 * (n - 1) - p if p >= n else p)


def _pad_sources(r, n, pad, mut):
    p = [r + pad]
    if 1 <= r <= pad:
        p.append(pad - r)
    if mut != "no_high_mirror" and n - 1 - pad <= r <= n - 2:
        p.append(pad + 2 * (n - 1) - r)
    return p


def _down_taps(r, n, no, mut):
    taps = []
    for q in _pad_sources(r, n, 1, mut):
        for t in range(3):
            e = q - t
            if e >= 0 and not e & 1 and (mut == "keep_ho" or (e >> 1) < no):
                taps.append((e >> 1, 2.0 if t == 1 else 1.0))
    return taps


def _up_taps(r, n, mut):
    taps = [(2 * r, 3.0), (2 * r + 1, 3.0)]
    if r + 1 < n:
        taps.append((2 * r + 2, 1.0))
    elif mut != "no_replicated_tap":
        taps.append((2 * n - 1, 1.0))
    if r >= 1:
        taps.append((2 * r - 1, 1.0))
    elif mut != "no_replicated_tap":
        taps.append((0, 1.0))
    return taps


def _axis_taps(op, n, pad, mut):
    """per output index of one axis: the (source index, weight) pairs in the kernel's order; n: the extent of the forward's input"""
    if op == "pad_fwd":
        return [[(_refl(i - pad, n, mut), 1.0)] for i in range(n + 2 * pad)]
    if op == "pad_bwd":
        return [[(q, 1.0) for q in _pad_sources(r, n, pad, mut)] for r in range(n)]
    if op == "down_fwd":
        no = (n - 1) // 2 + 1
        wt = (1.0, 1.0, 1.0) if mut == "w111" else (1.0, 2.0, 1.0)
        src = (lambda p: min(max(p, 0), n - 1)) if mut == "down_clamp" else (lambda p: _refl(p, n, mut))
        return [[(src(2 * y + t - 1), wt[t]) for t in range(3)] for y in range(no)]
    if op == "down_bwd":
        return [_down_taps(r, n, (n - 1) // 2 + 1, mut) for r in range(n)]
    if op == "up_fwd":
        out = []
        for o in range(2 * n):
            m, odd = o >> 1, bool(o & 1) != (mut == "up_phase")
            nb = m + 1 if odd else m - 1
            nb = _refl(nb, n, None) if mut == "up_mirror" else min(max(nb, 0), n - 1)
            out.append([(m, 3.0), (nb, 1.0)])
        return out
    return [_up_taps(r, n, mut) for r in range(n)]


def _tensors(taps):
    k = max(len(t) for t in taps)
    idx, w = torch.zeros(len(taps), k, dtype=torch.long), torch.zeros(len(taps), k)
    for i, t in enumerate(taps):
        for j, (s, ww) in enumerate(t):
            idx[i, j], w[i, j] = s, ww
    return idx, w


def emulate(op, v, H, W, pad=0, bf16=False, mut=None):
    """v: planes [B][h][w][C] fp32 (bf16: already bf16 values) -> the kernel's result, fp32 values. Reads go by flat address into the
    input followed by NaNs, as the kernel's address arithmetic would; an absent tap is weight 0 on element 0 (adds an exact zero)."""
    B, h, w, C = v.shape
    iy, wy = _tensors(_axis_taps(op, H, pad, mut))
    ix, wx = _tensors(_axis_taps(op, W, pad, mut))
    flat = torch.cat((v.float().reshape(-1), torch.full((4 * h * w * C + 64,), NAN)))
    b = torch.arange(B)[:, None, None, None]
    c = torch.arange(C)[None, None, None, :]
    acc = torch.zeros(B, len(iy), len(ix), C)
    for a in range(iy.shape[1]):
        r = torch.zeros_like(acc)
        for k in range(ix.shape[1]):
            addr = ((b * h + iy[:, a][None, :, None, None]) * w + ix[:, k][None, None, :, None]) * C + c
            t = torch.where(wx[:, k][None, None, :, None] != 0, flat[addr], torch.zeros(()))
            if op == "pad_bwd":                       # one flat sum over the (a, b) pairs
                acc = acc + torch.where(wy[:, a][None, :, None, None] != 0, t, torch.zeros(()))
            else:
                r = r + wx[:, k][None, None, :, None] * t
        if op != "pad_bwd":
            acc = acc + wy[:, a][None, :, None, None] * r
    if not op.startswith("pad"):
        acc = acc * (1.0 / 16.0)
    if bf16:
        acc = (acc.contiguous().view(torch.int32) & -65536).view(torch.float32) if mut == "trunc" else acc.bfloat16().float()
    if mut == "swap_pairs" and bf16 and C % 8 == 0:   # the halves of a packed pair the wrong way round in the 8-channel form
        acc = acc.view(B, len(iy), len(ix), C // 2, 2).flip(-1).reshape(B, len(iy), len(ix), C)
    return acc


def _check(op, shape, var, bf16, mut=None):
    """-> error / bound of the emulation on one case (exact: 0 or inf)"""
    B, C, H, W = shape
    pad = (br.exact_pad(shape) if var == "exact" else br.PADS.get(shape, 1)) if op.startswith("pad") else 0
    v = br.case(op, shape, var, pad)
    if bf16:
        v = v.bfloat16().float()
    ref, S = br.ref_of(op, v, H, W, pad, var)
    got = emulate(op, v, H, W, pad, bf16=bf16, mut=mut)
    if got.shape != ref.shape:
        return float("inf")
    if var == "exact" or op == "pad_fwd":
        return 0.0 if torch.equal(got.double(), ref) else float("inf")
    return br.ratio(got, ref, br.tolerance(op, ref, S, bf16))


@functools.lru_cache(maxsize=None)
def _impulse(op, H, W, pad, mut=None):
    """the emulation's impulse matrix (fp32), rows = impulses"""
    h, w = br.in_hw(op, H, W, pad)
    v = (16.0 * torch.eye(h * w)).view(h * w, h, w, 1)
    return emulate(op, v, H, W, pad, mut=mut).reshape(h * w, -1)


def _impulse_set(kind):
    s = [(h, w, p) for h, w in br.IMPULSE_HW for p in (range(1, min(h, w)) if kind == "pad" else (0,))]
    if kind == "up":
        s += [(h, w, 0) for h, w in br.IMPULSE_UP_EXTRA]
    return s


def _impulses_ok(kind, mut=None):
    for H, W, pad in _impulse_set(kind):
        f, b = _impulse(kind + "_fwd", H, W, pad, mut), _impulse(kind + "_bwd", H, W, pad, mut)
        if not (torch.equal(f, b.t()) and torch.equal(f.double(), br.impulse_reference(kind + "_fwd", H, W, pad))
                and torch.equal(b.double(), br.impulse_reference(kind + "_bwd", H, W, pad))):
            return False
    return True


@pytest.mark.parametrize("kind", ["pad", "down", "up"])
def test_emulated_impulse_matrices_are_the_references(kind):
    assert _impulses_ok(kind)
    assert any(p == h - 1 for h, w, p in _impulse_set("pad")) and (2, 2, 0) in _impulse_set("down")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_emulated_kernels_meet_the_definition(bf16):
    worst = {}
    for op in br.OPS:
        for shape in br.SHAPES + br.DISPATCH_SHAPES:
            assert _check(op, shape, "exact", bf16) == 0.0, (op, shape)
            q = _check(op, shape, "real", bf16)
            assert q <= 1.0, (op, shape, q)
            worst[op] = max(worst.get(op, 0.0), q)
    print("WORST emulation / bound", "bf16" if bf16 else "fp32", {k: float(f"{v:.4g}") for k, v in worst.items()})


# mutant -> (what must notice: 'impulse:<kind>' or (op, shape, variant, bf16))
MUTANTS = {
    "refl_repeat": "impulse:pad",
    "down_clamp": "impulse:down",
    "up_mirror": "impulse:up",
    "w111": "impulse:down",
    "up_phase": "impulse:up",
    "no_high_mirror": "impulse:pad",
    "keep_ho": "impulse:down",
    "no_replicated_tap": "impulse:up",
    "trunc": ("up_fwd", (1, 8, 33, 17), "real", True),
    "swap_pairs": ("down_fwd", (2, 24, 9, 12), "exact", True),
}


@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_mutant_is_rejected(mut):
    what = MUTANTS[mut]
    if isinstance(what, str):
        kind = what.split(":")[1]
        assert _impulses_ok(kind) and not _impulses_ok(kind, mut), f"the impulse matrices of {kind} do not notice {mut}"
        return
    op, shape, var, bf16 = what
    assert _check(op, shape, var, bf16) <= 1.0
    q = _check(op, shape, var, bf16, mut)
    print(mut, "on", what, q)
    assert not q <= 1.0, f"{what} does not notice {mut}"


def test_mutants_also_break_cases_with_data():
    """the border mutants move the exact cases and the bounds too, not only the impulse matrices"""
    for mut, op in (("refl_repeat", "pad_fwd"), ("down_clamp", "down_fwd"), ("up_mirror", "up_fwd"), ("w111", "down_fwd"), ("up_phase", "up_fwd"),
                    ("no_high_mirror", "pad_bwd"), ("no_high_mirror", "down_bwd"), ("keep_ho", "down_bwd"), ("no_replicated_tap", "up_bwd")):
        hit = [s for s in br.SHAPES if not _check(op, s, "exact", False, mut) <= 1.0 or not _check(op, s, "real", False, mut) <= 1.0]
        print(mut, op, "noticed on", hit)
        assert hit, (mut, op)
