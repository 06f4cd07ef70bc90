"""The definition of "correct" for the bilinear resize pair of csrc/augment.hip (resize_bilinear_kernel and its adjoint): a float64
reference built from exact bilinear weights, the bounds a correct kernel has to meet, and the shapes shared by tests/test_resize_ref.py
(CPU: proves reference and bounds on fp32 evaluations of the same operation) and tests/test_resize_gpu.py (the kernels themselves).
Plain torch, any device, no native code.

Per axis the operation is a matrix A[dst][src]: output index dst reads the source at s = max(n_src / n_dst * (dst + 1/2) - 1/2, 0), with
weight 1 - (s - floor s) on floor s and s - floor s on the next index, both on the last index once s passes it (align_corners = False).
    forward  out = A_y (x * mul + add) A_x^T            adjoint  dx = A_y^T dy A_x

What a correct kernel may do, with u = 2^-24, and what every coefficient below stands for:
  * the source index in fp32: the ratio is rounded (u), the product with dst + 1/2 (exact) is rounded (u), and so is the difference
    with 1/2 (u): 3 u (s + 1); C_IDX = 4 leaves one more for a kernel that forms the ratio or the half-pixel shift in another order.
                                                                                                        ds <= C_IDX u (s + 1)
  * the interpolant is continuous and piecewise linear in s, also across a floor that ds flips, and its slope is a difference of
    neighbouring source values: ds_y L_y + ds_x L_x, with L_y / L_x the image's largest vertical / horizontal neighbour difference.
  * values: x * mul and + add round once each (2 u of V = max(|x mul| + |add|)), 1 - lambda rounds on each axis (2 u), and the two-by-two
    combination is a product and a sum per axis (4 u): C_VAL = 8.               dout <= ds_y L_y + ds_x L_x + C_VAL u V
  * the adjoint: the weight of an output for a source index is a hat function of s with slope one, so an output within 1 + ds of a
    source index may move (ds_y + ds_x + C_W u) |dy| into it; C_W = 4: the two roundings of 1 - lambda and the two products. A source
    pixel that cnt outputs reach chains cnt fp32 additions: cnt u of the sum of |weight * dy|.
  * a bf16 result (BilinearResize on bf16 tensors) is rounded ONCE: 2^-8 |ref|.
"""
import torch

U = 2.0 ** -24
C_IDX, C_VAL, C_W = 4.0, 8.0, 4.0

# (h, w, H, W, batch)
SHAPES = [(5, 3, 64, 64, 3), (1, 1, 4, 5, 3), (7, 1, 1, 9, 3), (64, 48, 3, 5, 3), (3, 300, 5, 7, 3), (2, 257, 3, 600, 3), (33, 17, 33, 17, 3),
          (50, 70, 125, 91, 2), (304, 304, 1216, 1216, 1)]
# forward on the unit impulses == adjoint on the unit impulses, transposed
ADJOINT_SHAPES = [(5, 7, 12, 9), (12, 9, 5, 7), (4, 4, 16, 16), (16, 16, 4, 4), (40, 1, 3, 1), (1, 1, 3, 3), (2, 257, 2, 600), (3, 300, 2, 7)]


def axis(n_src, n_dst, device="cpu"):
    """-> A [n_dst][n_src] float64, ds [n_dst] (what the fp32 source index may be off by), reach [n_dst][n_src] (0 / 1: the outputs that a
    source index may get a share of)"""
    d = torch.arange(n_dst, dtype=torch.float64, device=device)
    s = ((n_src / n_dst) * (d + 0.5) - 0.5).clamp_min(0)
    i1 = s.floor().long().clamp_max(n_src - 1)
    lam = s - i1
    i2 = (i1 + 1).clamp_max(n_src - 1)
    A = torch.zeros(n_dst, n_src, dtype=torch.float64, device=device)
    rows = torch.arange(n_dst, device=device)
    A[rows, i1] += 1.0 - lam
    A[rows, i2] += lam
    ds = C_IDX * U * (s + 1.0)
    src = torch.arange(n_src, dtype=torch.float64, device=device)
    reach = ((src[None, :] - s[:, None]).abs() < 1.0 + ds[:, None]).double()
    return A, ds, reach


def values(x, mul=None, add=None):
    """x [B][h][w] -> (x * mul + add in float64, V [B])"""
    xd = x.double()
    m = mul.double()[:, None, None] if mul is not None else 1.0
    a = add.double()[:, None, None] if add is not None else 0.0
    return xd * m + a, ((xd * m).abs() + abs(a)).amax((1, 2))


def forward(x, H, W, mul=None, add=None, bf16=False):
    """-> (reference [B][H][W] float64, tolerance like it)"""
    B, h, w = x.shape
    v, V = values(x, mul, add)
    Ay, dsy, _ = axis(h, H, x.device)
    Ax, dsx, _ = axis(w, W, x.device)
    ref = torch.einsum("Yy,byx,Xx->bYX", Ay, v, Ax)
    zero = torch.zeros(B, dtype=torch.float64, device=x.device)
    Ly = (v[:, 1:] - v[:, :-1]).abs().amax((1, 2)) if h > 1 else zero
    Lx = (v[:, :, 1:] - v[:, :, :-1]).abs().amax((1, 2)) if w > 1 else zero
    tol = dsy[None, :, None] * Ly[:, None, None] + dsx[None, None, :] * Lx[:, None, None] + C_VAL * U * V[:, None, None]
    if bf16:
        tol = tol + 2.0 ** -8 * ref.abs()
    return ref, tol


def adjoint(dy, h, w, bf16=False):
    """dy [B][H][W] -> (reference [B][h][w] float64, tolerance like it)"""
    B, H, W = dy.shape
    Ay, dsy, Ry = axis(h, H, dy.device)
    Ax, dsx, Rx = axis(w, W, dy.device)
    d = dy.double()
    ref = torch.einsum("Yy,bYX,Xx->byx", Ay, d, Ax)
    moved = (dsy[None, :, None] + dsx[None, None, :] + C_W * U) * d.abs()
    cnt = torch.einsum("Yy,Xx->yx", Ry, Rx)
    tol = torch.einsum("Yy,bYX,Xx->byx", Ry, moved, Rx) + cnt * U * torch.einsum("Yy,bYX,Xx->byx", Ay, d.abs(), Ax)
    if bf16:
        tol = tol + 2.0 ** -8 * ref.abs()
    return ref, tol


def ratio(got, ref, tol):
    """the largest error / bound; an error where the bound is 0, or a NaN, counts as inf"""
    got = got.double().reshape(ref.shape)
    err = (got - ref).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / tol)
    q = torch.where(torch.isnan(got), torch.full_like(q, float("inf")), q)
    return q.max().item()


def case(shape, device="cpu"):
    """-> x [B][h][w] fp32, x8 uint8 like it, dy [B][H][W], mul, add [B] (add nonzero)"""
    h, w, H, W, B = shape
    gen = torch.Generator().manual_seed(5000 + h * 7 + w * 11 + H * 13 + W * 17)
    x = torch.randn(B, h, w, generator=gen) * 3.0 + 1.0
    x8 = torch.randint(0, 256, (B, h, w), generator=gen, dtype=torch.uint8)
    dy = torch.randn(B, H, W, generator=gen)
    mul = torch.rand(B, generator=gen) + 0.5
    add = torch.rand(B, generator=gen) * 2.0 + 1.0
    return tuple(t.to(device) for t in (x, x8, dy, mul, add))
