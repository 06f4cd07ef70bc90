"""The definition of "correct" for the six kernels of csrc/blur.hip (reflection pad, [1 2 1]^2 blur-downsample, [1 3 3 1]^2 blur-upsample,
each with its hand-gathered backward): float64 references by explicit index arithmetic, the two families of inputs they are applied to, the
bound a correct kernel has to meet on the second family, and the shapes shared by tests/test_blur_ref.py (CPU: proves references and bounds
on an fp32 emulation of each kernel) and tests/test_blur_exact_gpu.py (the kernels themselves). Plain torch, any device, no native code, and
no torch convolution: the references are independent of the torch expressions tests/test_blur_gpu.py compares with (tests/test_blur_ref.py
checks the two against each other in float64). ratio() comes from tests/_conv_ref.py.

Each operation is separable: a matrix A[out][in] per axis, filled index by index with the closed forms of the kernel file's header,
    pad  : A[i][refl(i - pad)] = 1,                                  i < n + 2 pad,  refl(p) = -p below 0, 2 (n - 1) - p from n on (mirror without
                                                                                     repeating the border)
    down : A[y][refl(2 y + t - 1)] += k3[t],  k3 = [1 2 1] / 4,      y < (n - 1) / 2 + 1
    up   : A[2 m][m] += 3/4, A[2 m][max(m - 1, 0)] += 1/4,  A[2 m + 1][m] += 3/4, A[2 m + 1][min(m + 1, n - 1)] += 1/4   (clamp: a replicated border)
    forward  out = A_y x A_x^T  per plane and channel          backward  dx = A_y^T g A_x
on planes [B][H][W][C] (an NCHW tensor is B * C planes of one channel). Every entry of A is >= 0, so S, the sum of the magnitudes of the
terms of an output, is the same operator applied to |x|.

EXACT cases. Inputs 16 k, k an integer in [-3, 3]. The forward weights of an output sum to 16/16 and the transposed weights of the
blurs to at most 64/16, all of them multiples of 1/16: every output is an integer, and reference() of an exact case asserts that its
magnitude stays <= 192. The pad's backward adds one input per padded position that reads the pixel: up to 3 per axis where the two
mirrors overlap, which could reach 9 * 48; the exact cases therefore use exact_pad(), the largest pad (up to the case's own) at which
no index has both mirrors: at most 2 x 2 inputs (an axis of 3 has no such pad; pad 1 then, and the assertion decides). The largest pad H - 1 runs in the real-valued cases and the impulse matrices. Integers of
that size, and every partial sum of the kernels (multiples of 16 below 2^24 before the factor 1/16), are fp32 AND bf16 numbers: one legal
result in both dtypes and both layouts, compared with torch.equal.

IMPULSES. The operator applied to the unit impulses times 16 gives 16 A_y (x) A_x, entry by entry exact in both dtypes; the backward's
matrix has to be the exact transpose of the forward's and both have to be the reference's. Over every (H, W) with H, W in 2..6 (and the
largest pad H - 1) this pins pad_sources, down_taps and up_taps at every border configuration.

REAL-VALUED cases (N(0, 1)). Every element: |got - ref| <= D * 2^-24 * S in fp32, plus 2^-8 |ref| in bf16 (arithmetic is fp32, rounded once
on store). D counts the dependent fp32 roundings behind one output, read from each kernel (a compiler that contracts a product and a sum
into one fused operation rounds less often, never more):
  pad fwd   a copy: no arithmetic, compared with torch.equal.
  pad bwd   acc += t over at most 3 x 3 sources, the first into zero:                                                    D = 8
  down fwd  per row r0 + 2 r1 + r2 (the doubling is exact): 2; acc += {1, 2} r over three rows, the first into zero: 2;
            the factor 1/16 is exact:                                                                                    D = 4
  down bwd  down_taps yields at most 3 sources x 2 taps of the right parity = 6 per axis; r += wx t (wx in {1, 2}: exact products): 5
            after the first, acc += wy r: 5 after the first:                                                             D = 10
  up fwd    (3 (3 a + b) + (3 c + d)) / 16: 3 a, + b, 3 (.), the last sum:                                               D = 4
  up bwd    four taps per axis; r += wx t with wx = 3 a rounded product: 1 + 4 (the first sum into zero counts: its product rounded),
            acc += wy r: 1 + 4:                                                                                          D = 10

THE DISPATCH, as read from OCTA_BLUR_LAUNCH: fp32 runs the scalar form; bf16 runs the 8-channels-per-thread form where C % 8 == 0 and both
pointers are 16-byte aligned, else the scalar form. NOT COVERED: the 64-bit branch of split() needs a tensor of more than 2^31 elements,
which no test of a few seconds reaches.
"""
import functools

import torch

from _conv_ref import HALF_BF16, U24, ratio  # noqa: F401  (ratio: for the users of this module)

OPS = ("pad_fwd", "pad_bwd", "down_fwd", "down_bwd", "up_fwd", "up_bwd")
ENTRY = {"pad_fwd": "octa_reflect_pad_fwd", "pad_bwd": "octa_reflect_pad_bwd", "down_fwd": "octa_blur_down_fwd", "down_bwd": "octa_blur_down_bwd",
         "up_fwd": "octa_blur_up_fwd", "up_bwd": "octa_blur_up_bwd"}
D = {"pad_fwd": 0, "pad_bwd": 8, "down_fwd": 4, "down_bwd": 10, "up_fwd": 4, "up_bwd": 10}
EXACT_LIMIT = 192.0

# [B][C][H][W] of the real-valued and the exact cases (four of tests/test_blur_gpu.py's: odd sizes, H = 2, more than one block, C % 8 == 0); the pad of each
SHAPES = [(1, 5, 7, 10), (2, 4, 2, 3), (1, 8, 33, 17), (2, 24, 9, 12)]
PADS = {(1, 5, 7, 10): 3, (2, 4, 2, 3): 1, (1, 8, 33, 17): 3, (2, 24, 9, 12): 8}
# the impulse matrices: every border configuration of a short axis
IMPULSE_HW = [(h, w) for h in range(2, 7) for w in range(2, 7)]
IMPULSE_UP_EXTRA = [(1, 1), (1, 5), (9, 2)]
# the dispatch of the bf16 forms: C % 8 == 0 (vector form where aligned), and C = 12 (scalar form at an aligned address)
DISPATCH_SHAPES = [(2, 8, 5, 6), (1, 24, 4, 7), (1, 12, 5, 4)]


def exact_pad(shape):
    """the pad of a shape's EXACT pad cases: the largest one <= PADS[shape] (1 for a shape without an entry) at which no index of either axis
    is read through both mirrors (pad_sources: 1 <= r <= pad and n - 1 - pad <= r <= n - 2)"""
    for pad in range(PADS.get(shape, 1), 0, -1):
        if all(max(1, n - 1 - pad) > min(pad, n - 2) for n in shape[2:]):
            return pad
    return 1                    # an axis of 3 has both mirrors on its middle index at any pad: 2 x 3 inputs, and ref_of() still asserts the limit


def refl(p, n):
    return -p if p < 0 else (2 * (n - 1) - p if p >= n else p)


def axis(kind, n, pad=0):
    """-> A [n_out][n] float64 of one axis of `kind` = pad | down | up (module docstring)"""
    if kind == "pad":
        A = torch.zeros(n + 2 * pad, n, dtype=torch.float64)
        for i in range(n + 2 * pad):
            A[i, refl(i - pad, n)] = 1.0
    elif kind == "down":
        A = torch.zeros((n - 1) // 2 + 1, n, dtype=torch.float64)
        for y in range(A.shape[0]):
            for t, k in enumerate((0.25, 0.5, 0.25)):
                A[y, refl(2 * y + t - 1, n)] += k
    else:
        A = torch.zeros(2 * n, n, dtype=torch.float64)
        for m in range(n):
            A[2 * m, m] += 0.75
            A[2 * m, max(m - 1, 0)] += 0.25
            A[2 * m + 1, m] += 0.75
            A[2 * m + 1, min(m + 1, n - 1)] += 0.25
    return A


def out_hw(op, H, W, pad=0):
    kind = op.split("_")[0]
    return {"pad": (H + 2 * pad, W + 2 * pad), "down": ((H - 1) // 2 + 1, (W - 1) // 2 + 1), "up": (2 * H, 2 * W)}[kind]


def reference(op, v, H, W, pad=0):
    """v: planes [B][h][w][C] (the input of a forward operation, the gradient of its output for a backward one); H, W: the extent of the
    forward's INPUT -> (ref, S) float64"""
    kind, way = op.split("_")
    Ay, Ax = axis(kind, H, pad).to(v.device), axis(kind, W, pad).to(v.device)
    v = v.double()
    eq = "Yy,byxc,Xx->bYXc" if way == "fwd" else "Yy,bYXc,Xx->byxc"
    assert v.shape[1:3] == ((H, W) if way == "fwd" else out_hw(op, H, W, pad)), (op, v.shape, H, W)
    return torch.einsum(eq, Ay, v, Ax), torch.einsum(eq, Ay, v.abs(), Ax)


def tolerance(op, ref, S, bf16):
    tol = D[op] * U24 * S
    return tol + HALF_BF16 * ref.abs() if bf16 else tol


def in_hw(op, H, W, pad=0):
    """the extent of the tensor the kernel of `op` READS, for a forward input of H x W"""
    return (H, W) if op.endswith("fwd") else out_hw(op, H, W, pad)


@functools.lru_cache(maxsize=None)
def case(op, shape, var, pad=0):
    """-> planes [B][h][w][C] fp32 on the CPU (channels last; the NCHW form of the same data is its permutation), drawn from a generator
    seeded per case: 16 k with k in [-3, 3] (exact) or N(0, 1) (real; the bf16 runs round it first)"""
    B, C, H, W = shape
    h, w = in_hw(op, H, W, pad)
    gen = torch.Generator().manual_seed(9000 + 13 * OPS.index(op) + 101 * H + 7 * W + C + (var == "real"))
    if var == "exact":
        return torch.randint(-3, 4, (B, h, w, C), generator=gen).float() * 16.0
    return torch.randn((B, h, w, C), generator=gen)


def ref_of(op, v, H, W, pad, var):
    """reference() of a case; an exact case asserts its premise"""
    ref, S = reference(op, v, H, W, pad)
    if var == "exact":
        assert torch.equal(ref, ref.round()) and ref.abs().max().item() <= EXACT_LIMIT and S.max().item() * 16 < 2.0 ** 24, \
            f"{op}: outputs reach {ref.abs().max().item()}"
    return ref, S


def impulse_reference(op, H, W, pad=0):
    """16 * (A_y (x) A_x) [inputs][outputs] for a forward op, its transpose [outputs][inputs] for the backward one: row i is the operator's
    answer to 16 * the i-th unit impulse"""
    kind, way = op.split("_")
    M = 16.0 * torch.kron(axis(kind, H, pad), axis(kind, W, pad))           # [Ho * Wo][H * W]
    return M.t().contiguous() if way == "fwd" else M


def refusals(H=4, W=5):
    """calls the host code has to refuse: name -> (op family or None for all six, dtype, B, H, W, C, pad, alias)"""
    return {"pad_0": ("pad", 0, 1, H, W, 2, 0, False), "pad_eq_h": ("pad", 0, 1, H, W, 2, H, False), "pad_eq_w": ("pad", 1, 1, W, H, 2, H, False),
            "down_h1": ("down", 0, 1, 1, W, 2, 0, False), "down_w1": ("down", 1, 1, H, 1, 2, 0, False), "dtype_2": (None, 2, 1, H, W, 2, 1, False),
            "alias": (None, 0, 1, H, W, 2, 1, True), "b_0": (None, 1, 0, H, W, 2, 1, False), "c_0": (None, 0, 1, H, W, 0, 1, False)}
