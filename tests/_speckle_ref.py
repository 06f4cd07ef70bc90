"""The definition of "correct" for the speckle passes of csrc/augment.hip (octa_speckle_brightness: speckle_pass1_kernel, the per-image
extrema through order-preserving integer atomics, speckle_pass2_kernel): a float64 reference, the bound a correct kernel has to meet,
and the cases shared by tests/test_speckle_ref.py (CPU) and tests/test_speckle_gpu.py (the kernels). Plain torch, any device, no native
code.

    C = the 9 x 9 control grid resized bilinearly to H x W (align_corners = False)       R = C - u (1 - C)       v = img R
    out = v / max v - min v / max v,  the extrema per image

C is _resize_ref.forward on the grids; its tolerance tol_C is the resize bound already proved. From there, with u_ = 2^-24 for one fp32
rounding and first-order terms only, as in _resize_ref:
  * 1 - C rounds once: tol_C + u_ |1 - C|; its product with u rounds once: |u| tol_C + 2 u_ |u (1 - C)|; the difference with C once:
                                                                dR <= (1 + |u|) tol_C + u_ (2 |u (1 - C)| + |R|)
  * img is given in fp32 and the product rounds once:                          dv <= |img| dR + u_ |v|
  * the extrema of the computed v are off by at most D = max dv of the image: |dmax|, |dmin| <= D. The bound needs max v > D (asserted):
    the all-zero image divides by zero in the reference as well and is no part of the contract.
  * a quotient p / max with p off by dp: (dp + |p / max| D) / (max - D), and one rounding, u_ |p / max|. For p = v that is
    (dv + |q| D) / (max - D) + u_ |q|, for p = min (D + |q_min| D) / (max - D) + u_ |q_min|; the difference rounds once more, u_ |out|.
                                        dout <= (dv + (1 + |q| + |q_min|) D) / (max - D) + u_ (|q| + |q_min| + |out|)
Exact, with no tolerance: the pixel that holds the minimum and the minimum the atomics deliver are the same float, the two quotients
the same, and division by a positive number is monotone: out.min() of every image is exactly 0, nothing is NaN; integer atomics do not
depend on their order, so two runs give equal bits.

Largest error / bound of the fp32 emulation of tests/test_speckle_ref.py (CPU):
    0.068 (3 x 33 x 257, isolation), 0.068 as well with the minimum subtracted first. Most of the bound is tol_C, the resize bound's
    allowance for the source index times the grid's largest neighbour difference.
"""
import functools

import torch

import _resize_ref as rr

U = 2.0 ** -24
# (B, H, W): one pixel; the grid's own size; a width across the 256-thread block; the parity test's shape; odd sizes with a second block
SHAPES = [(1, 1, 1), (3, 9, 9), (3, 7, 300), (2, 64, 80), (3, 33, 257)]
VARIANTS = ("plain", "grid outside", "negative", "isolation")

ratio = rr.ratio


def reference(img, grid9, u):
    """img, u [B][H][W], grid9 [B][9][9] -> (reference float64, tolerance like it)"""
    B, H, W = img.shape
    C, tol_c = rr.forward(grid9, H, W)
    i, uu = img.double(), u.double()
    R = C - uu * (1.0 - C)
    v = i * R
    dR = (1.0 + uu.abs()) * tol_c + U * (2.0 * (uu * (1.0 - C)).abs() + R.abs())
    dv = i.abs() * dR + U * v.abs()
    D = dv.amax((1, 2), keepdim=True)
    mx, mn = v.amax((1, 2), keepdim=True), v.amin((1, 2), keepdim=True)
    assert bool((mx > 2.0 * D).all()), "max v must be positive, and by more than the rounding of v"
    q, qm = v / mx, mn / mx
    ref = q - qm
    tol = (dv + (1.0 + q.abs() + qm.abs()) * D) / (mx - D) + U * (q.abs() + qm.abs() + ref.abs())
    return ref, tol


@functools.lru_cache(maxsize=None)
def cases(shape):
    """-> [(name, img, grid9, u)] on the CPU. plain: img in [0, 1], grid in [0.5, 1) as the transform draws it; grid outside: grid in [1, 2);
    negative: pixels in [-0.5, 1) around a positive maximum (the order map's branch for negative floats, a negative minimum);
    isolation: image b in [0, 1e-3] next to image b + 1 in [0, 100]."""
    B, H, W = shape
    g = torch.Generator().manual_seed(9000 + 7 * H + 11 * W)
    out = []
    for name in VARIANTS:
        img = torch.rand(B, H, W, generator=g) * 0.9 + 0.1
        grid = torch.rand(B, 9, 9, generator=g) * 0.5 + 0.5
        u = torch.rand(B, H, W, generator=g)
        if name == "grid outside":
            grid = grid * 2.0
        elif name == "negative":
            if H * W == 1:
                continue
            img = torch.rand(B, H, W, generator=g) * 1.5 - 0.5
            img[:, 0, 0] = 0.75
        elif name == "isolation":
            if B < 2:
                continue
            img = torch.rand(B, H, W, generator=g) * torch.tensor([1e-3 if b % 2 == 0 else 100.0 for b in range(B)])[:, None, None]
        out.append((name, img.contiguous(), grid.contiguous(), u.contiguous()))
    return out
