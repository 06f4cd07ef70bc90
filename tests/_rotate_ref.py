"""The definition of "correct" for rotate_kernel and rotate_window_kernel of csrc/augment.hip (octa_flip_rot90_rotate and its window form):
a float64 reference, the bounds a correct kernel has to meet, and the cases shared by tests/test_rotate_ref.py (CPU: proves reference and
bounds on fp32 evaluations of the same operation) and tests/test_rotate_gpu.py (the kernels themselves). Plain torch, any device, no
native code.

The operation, per image: torch.flip(x, (0, 1)) if flip, torch.rot90(., k, (0, 1)), then the rotation by `angle` about the image centre
with bilinear taps and zeros outside. The reference samples the flipped / turned image y at the CENTRED coordinates
    fx = c (X - m) - s (Y - m) + m      fy = s (X - m) + c (Y - m) + m      m = (N - 1) / 2,  c = cos angle,  s = sin angle
with floor, four taps and zeros outside [0, N)^2. That is algebraically the kernel's affine_grid / grid_sample chain
(g = (2 i + 1) / N - 1, the rotation of g, ((. + 1) N - 1) / 2) but not its sequence of operations. The window form is a slice of the
zero-extended result; a threshold (AsDiscrete) is applied after the extension.

What a correct kernel may do, with u = 2^-24, in the order of the kernel's expressions. Coordinates are in grid_sample's normalised
units (the frame is [-1, 1]) until the last step; |g| <= 1, |c| + |s| <= sqrt 2, |c g_x| + |s g_y| <= sqrt 2, |sx| <= sqrt 2.
  * cosf, sinf: k ulp each, and an ulp of v is at most 2 u |v|: dc <= 2 k u |c|, ds <= 2 k u |s|. k = TRIG_ULP = 4: the device library
    (ROCm's OCML) implements the OpenCL C accuracy table, which allows sin and cos 4 ulp (OpenCL C specification, "Relative error as
    ULPs"); the single-precision table of the HIP math API reference lists sinf and cosf at 1 ulp, as measured rather than promised.
    The larger figure is taken.
  * g = (2 i + 1) / N - 1: 2 i + 1 is exact, the quotient (below 2) rounds once, 2 u, the difference once, u: dg <= 3 u.
  * sx = c g_x - s g_y: the inputs' errors, (|c| + |s|) 3 u + 2 k u (|c g_x| + |s g_y|) <= sqrt 2 (3 + 2 k) u, the two products,
    u (|c g_x| + |s g_y|) <= sqrt 2 u, and the difference, u |sx| <= sqrt 2 u. A contraction to an fma only removes a rounding.
                                                                                                        dsx <= sqrt 2 (5 + 2 k) u
  * fx = ((sx + 1) N - 1) 0.5: sx + 1 rounds once, (1 + sqrt 2) u; the product with N carries both to N (dsx + (1 + sqrt 2) u) and rounds
    once, (1 + sqrt 2) N u; - 1 rounds once, ((1 + sqrt 2) N + 1) u; the half is exact and turns the unit into pixels:
        dfx <= (N u / 2) (sqrt 2 (5 + 2 k) + 3 (1 + sqrt 2)) + u / 2 = 12.82 N u + u / 2      for k = 4
  * tx = fx - floor fx is exact except for fx in (-1, 0), where it is fx + 1 and rounds once, u: a move of the coordinate as well.
    Together: ds <= C_COORD u (N + 1), C_COORD = 13, the same for both axes. (A plain fp32 evaluation reaches 3.3 u N.)
  * the interpolant of the zero-extended image is continuous and piecewise bilinear, also across a floor that ds flips; its slope along
    an axis is a convex combination of neighbour differences along that axis. The output moves by at most ds (L_y + L_x), L the largest
    vertical / horizontal neighbour difference of the image ZERO-PADDED BY ONE PIXEL (further out every difference is 0). Flip and
    rot90 permute or swap the two, so L_y + L_x is taken from the stored image.
  * values: 1 - tx and 1 - ty round once each, a weight is their product (3 u on a weight), tap * weight rounds once (4 u), and the first
    term goes through three additions (7 u); the weights are positive and sum to at most 1: C_VAL = 8 of V = max |x|.
                                                                                    dout <= ds (L_y + L_x) + C_VAL u V
  * an output whose reference coordinate lies further than 1 + ds in front of the frame or ds behind it on either axis has all four taps
    outside whatever the kernel's roundings did: it is EXACTLY 0 (tolerance 0), and so is the padding of the window form.
  * thresholded output: a pixel is DECIDED when |ref - threshold| > tol (or tol = 0); there the kernel gives exactly ref >= threshold. An
    undecided pixel may be 0 or 1 and nothing else. caps() states, on the reference alone, that the undecided pixels are at most 0.5 %
    of each image and that each image keeps N decided ones and N decided zeros. An image of N <= 2 has fewer than 2 N pixels to give
    (N = 1) or single pixels of 25 % (N = 2): there no pixel at all may be undecided, and the BATCH holds a decided one and a decided zero.

Largest error / bound of the fp32 evaluations of tests/test_rotate_ref.py (CPU):
    torch's fp32 grid_sample 0.100, the emulation of rotate_kernel 0.107 (both at N = 257, the constant image; N = 304: 0.097 and 0.101).
    The bound is about ten times what these evaluations need: it adds up the worst case of every rounding, a third of C_COORD for the
    4 ulp allowed to sinf / cosf alone. Every mutant of tests/test_rotate_ref.py still breaks it, or the exact check.
    Undecided pixels of the thresholded cases: at most 0.37 % of an image (random image, threshold 0.5, N = 304), 0.10 % on the label.
"""
import functools
import math

import torch
import torch.nn.functional as F

import _resize_ref as rr

U = 2.0 ** -24
TRIG_ULP = 4.0
C_COORD, C_VAL = 13.0, 8.0
assert 0.5 * (math.sqrt(2.0) * (5.0 + 2.0 * TRIG_ULP) + 3.0 * (1.0 + math.sqrt(2.0))) <= C_COORD and 1.5 <= C_COORD      # N u and u parts

SIZES = [1, 2, 31, 32, 37, 255, 256, 257, 304]
ANGLES = [0.0, 0.1745, -0.093, 0.7854, 3.0]
KINDS = ("random", "label", "ones", "ramp")
THRESHOLD = {"label": 0.1, "random": 0.5}
UNDECIDED_CAP = 0.005

ratio = rr.ratio


def permute(x, rot_k=None, flip=None):
    """x [B][N][N] -> torch.flip(., (0, 1)) where flip, then torch.rot90(., k, (0, 1)), image by image"""
    out = []
    for b in range(x.shape[0]):
        y = x[b]
        if flip is not None and int(flip[b]):
            y = torch.flip(y, (0, 1))
        out.append(torch.rot90(y, int(rot_k[b]) if rot_k is not None else 0, (0, 1)))
    return torch.stack(out)


def coords(N, angle, device):
    """-> fx, fy [B][N][N] float64: where output pixel (Y, X) reads the flipped / turned image"""
    m = (N - 1) / 2.0
    i = torch.arange(N, dtype=torch.float64, device=device) - m
    Y, X = i[None, :, None], i[None, None, :]
    a = angle.to(device=device, dtype=torch.float64)[:, None, None]
    c, s = torch.cos(a), torch.sin(a)
    return c * X - s * Y + m, s * X + c * Y + m


def sample(y, fx, fy):
    """bilinear taps of y [B][N][N] float64 at (fy, fx), zeros outside"""
    B, N, _ = y.shape
    x0, y0 = fx.floor(), fy.floor()
    tx, ty = fx - x0, fy - y0
    flat = y.reshape(B, N * N)

    def tap(iy, ix):
        ok = (iy >= 0) & (iy < N) & (ix >= 0) & (ix < N)
        idx = (iy.clamp(0, N - 1) * N + ix.clamp(0, N - 1)).long().reshape(B, -1)
        return torch.gather(flat, 1, idx).reshape(iy.shape) * ok

    return (tap(y0, x0) * (1 - tx) * (1 - ty) + tap(y0, x0 + 1) * tx * (1 - ty) + tap(y0 + 1, x0) * (1 - tx) * ty + tap(y0 + 1, x0 + 1) * tx * ty)


def coord_error(N):
    return C_COORD * U * (N + 1)


def window(t, size, offs, fill=0.0):
    """t [B][N][N] -> [B][size[0]][size[1]]: rows oy .. oy + size[0], columns ox .. ox + size[1] of image b extended by `fill`"""
    N = t.shape[1]
    P = max([0] + [-o for oo in offs for o in oo] + [oy + size[0] - N for oy, _ in offs] + [ox + size[1] - N for _, ox in offs])
    ext = F.pad(t, (P, P, P, P), value=fill)
    return torch.stack([ext[b, P + oy:P + oy + size[0], P + ox:P + ox + size[1]] for b, (oy, ox) in enumerate(offs)])


def reference(x, angle, rot_k=None, flip=None, win=None, extra=0.0):
    """x [B][N][N], angle [B] float32 -> (reference BEFORE any threshold, float64, and a tolerance like it). win = (size, [(oy, ox)] * B):
    the window form. extra: what x itself may be off by, when it is the output of another kernel (the weights sum to at most 1)."""
    B, N, _ = x.shape
    xd = x.double()
    fx, fy = coords(N, angle, x.device)
    ref = sample(permute(xd, rot_k, flip), fx, fy)
    ds = coord_error(N)
    pad = F.pad(xd, (1, 1, 1, 1))
    L = (pad[:, 1:] - pad[:, :-1]).abs().amax((1, 2)) + (pad[:, :, 1:] - pad[:, :, :-1]).abs().amax((1, 2)) + 4.0 * extra
    V = xd.abs().amax((1, 2)) + extra
    dead = (fx < -1 - ds) | (fx >= N + ds) | (fy < -1 - ds) | (fy >= N + ds)
    tol = torch.where(dead, torch.zeros_like(ref), (ds * L + C_VAL * U * V + extra)[:, None, None].expand_as(ref))
    if win is not None:
        ref, tol = window(ref, *win), window(tol, *win)
    return ref, tol


def decided(ref, tol, thr):
    return ((ref - thr).abs() > tol) | (tol == 0)


def discrete(got, ref, tol, thr):
    """the thresholded output against the rule -> (decided pixels that are not ref >= thr, values that are neither 0 nor 1)"""
    got = got.reshape(ref.shape)
    want = (ref >= thr).to(got.dtype)
    return int(((got != want) & decided(ref, tol, thr)).sum()), int(((got != 0) & (got != 1)).sum())


def caps(ref, tol, thr, classes=True):
    """The conditions a thresholded case has to meet before it can test anything, from the reference alone -> (largest undecided share
    of an image, fewest decided ones, fewest decided zeros of an image); asserts them. classes = False: the share only (a window at
    threshold 0 has no zeros to show)."""
    B, N = ref.shape[0], ref.shape[-1]
    d = decided(ref, tol, thr)
    per = ref.shape[1] * ref.shape[2]
    undecided = (~d).sum((1, 2))
    ones, zeros = (d & (ref >= thr)).sum((1, 2)), (d & (ref < thr)).sum((1, 2))
    share = float(undecided.max()) / per
    assert int(undecided.max()) <= UNDECIDED_CAP * per, ("undecided", undecided.tolist(), per)
    if not classes:
        pass
    elif N > 2:
        assert int(ones.min()) >= N and int(zeros.min()) >= N, ("decided ones / zeros", ones.tolist(), zeros.tolist(), N)
    else:
        assert int(ones.sum()) >= 1 and int(zeros.sum()) >= 1, ("decided ones / zeros in the batch", ones.tolist(), zeros.tolist())
    return share, int(ones.min()), int(zeros.min())


# ---- the shared cases -------------------------------------------------------------------------------------------------------------------

def batch(N):
    return 8 if N in (32, 37) else 3          # eight: all (k, flip) pairs in one launch


def image(kind, N, B):
    g = torch.Generator().manual_seed(7000 + 13 * N + KINDS.index(kind))
    if kind == "random":
        return torch.randn(B, N, N, generator=g) * 0.5 + 0.5
    if kind == "label":
        x = (torch.rand(B, N, N, generator=g) < 0.3).float()
        if N <= 2:                              # four pixels at most: one image with a vessel pixel for certain, one without any
            x[0, 0, 0], x[1] = 1.0, 0.0
        return x
    if kind == "ones":
        return torch.ones(B, N, N)
    i = torch.arange(N, dtype=torch.float32)            # slopes in 1024ths: every value is exact in fp32, the ramp is a ramp to the last bit
    a, b = (torch.arange(B) % 4 + 1).float() / 1024.0, -(torch.arange(B) % 3 + 2).float() / 1024.0
    return (a[:, None, None] * i[None, None, :] + b[:, None, None] * i[None, :, None]).contiguous()


@functools.lru_cache(maxsize=None)
def cases(N):
    """-> [(name, kind, x [B][N][N] fp32, angle [B] fp32, rot_k, flip int32 [B] or None)], on the CPU. Two launches per image kind walk the five
    angles and the (k, flip) pairs; the random image also goes without the two tables."""
    B = batch(N)
    out = []
    for kind in KINDS:
        x = image(kind, N, B)
        for grp in (0, 1):
            b = torch.arange(B)
            angle = torch.tensor([ANGLES[(3 * grp + int(i)) % 5] for i in b], dtype=torch.float32)
            if B == 8:
                k, f = (b // 2 + grp) % 4, b % 2
            else:
                k, f = (b + grp + N) % 4, (b + grp) % 2
            out.append((f"{kind} g{grp}", kind, x, angle, k.int(), f.int()))
            if kind == "random":
                out.append((f"{kind} g{grp} no tables", kind, x, angle, None, None))
    return out


def to(device, *ts):
    return tuple(t.to(device) if t is not None else None for t in ts)


# the window geometry of tests/test_crop_gpu.py: (N, (out_h, out_w), per-image (oy, ox)); B = 3
WINDOW_CASES = {
    "corner00": (37, (13, 20), [(0, 0)] * 3),
    "corner_far": (37, (13, 20), [(37 - 13, 37 - 20)] * 3),
    "interior": (37, (13, 20), [(3, 11), (17, 2), (9, 9)]),
    "block_seam": (300, (280, 290), [(0, 0), (20, 10), (7, 3)]),
    "pad": (37, (48, 48), [(-5, -5)] * 3),
}
WINDOW_ANGLES = [0.1745, -0.093, 0.7854]
WINDOW_THRESHOLDS = (None, 0.1, 0.0)


@functools.lru_cache(maxsize=None)
def window_case(name):
    """-> x [3][N][N] fp32 in (0, 1), angle, rot_k, flip, on the CPU"""
    N, size, offs = WINDOW_CASES[name]
    g = torch.Generator().manual_seed(N * 1000 + size[0])
    x = torch.rand((3, N, N), generator=g) * 0.9 + 0.1
    return x, torch.tensor(WINDOW_ANGLES, dtype=torch.float32), torch.tensor([1, 3, 2], dtype=torch.int32), torch.tensor([1, 0, 1], dtype=torch.int32)
