"""2-D skeletonisation for the clDice metric (reference utils/cldice.py: `skimage.morphology.skeletonize`): Zhang & Suen's 1984
parallel thinning, restated from the published rule.

For a foreground pixel P1 with the neighbours clockwise from north P2 = N, P3 = NE, P4 = E, P5 = SE, P6 = S, P7 = SW, P8 = W, P9 = NW
(outside the image = background), B = number of non-zero neighbours and A = number of 0 -> 1 steps in the cyclic sequence P2 .. P9, P2,
the pixel is removable when 2 <= B <= 6 and A == 1 and
    first sub-iteration:  P2 P4 P6 == 0 and P4 P6 P8 == 0        second sub-iteration: P2 P4 P8 == 0 and P2 P6 P8 == 0.
A sub-iteration decides every pixel on the image as it was when it began and removes all removable pixels at once; (first, second)
repeats until a whole double pass removes nothing.

`skeletonize_device` runs csrc/skeleton.hip (bit-packed words, bitwise logic) on CUDA tensors, `skeletonize_host` is the same rule in
numpy (neighbour code from eight shifted views, table lookup) for CPU tensors and as the tests' full-size reference. There is no
route from a CUDA tensor to the host version: `skeletonize` sends every CUDA tensor to the kernel, whatever its dtype or strides.

Parity with scikit-image itself is UNPINNED: scikit-image is neither installed where this project is built nor shipped with the
reference (the same standing as `skimage.draw.line`). What pins the rule is the published algorithm, a literal
per-pixel oracle in tests/test_skeleton.py and the known answers there."""
import ctypes

import numpy as np
import torch

# neighbour k of the code's bit k: (dy, dx) of P2 .. P9
NEIGHBOURS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))


def removal_tables():
    """(first, second): bool [256], indexed by the neighbour code sum(P(2 + k) << k), True where the rule removes the pixel."""
    code = np.arange(256)
    p = [(code >> k) & 1 for k in range(8)]                      # p[0] = P2 ... p[7] = P9
    b = sum(p)
    a = sum((1 - p[k]) * p[(k + 1) % 8] for k in range(8))
    common = (b >= 2) & (b <= 6) & (a == 1)
    p2, p4, p6, p8 = p[0], p[2], p[4], p[6]
    first = common & (p2 * p4 * p6 == 0) & (p4 * p6 * p8 == 0)
    second = common & (p2 * p4 * p8 == 0) & (p2 * p6 * p8 == 0)
    return first, second


_TABLES = removal_tables()


def _neighbour_code(img):
    """uint8 [H, W]: the code of every pixel, from eight shifted views of the zero-padded image."""
    h, w = img.shape
    pad = np.zeros((h + 2, w + 2), dtype=np.uint8)
    pad[1:-1, 1:-1] = img
    code = np.zeros((h, w), dtype=np.uint8)
    for k, (dy, dx) in enumerate(NEIGHBOURS):
        code |= pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] << k
    return code


def skeletonize_host(array, return_passes=False):
    """numpy restatement of the rule: array [H, W] of any dtype (non-zero = foreground) -> uint8 [H, W] of 0 / 1. With return_passes
    also the number of double passes that removed something."""
    img = (np.asarray(array) != 0).astype(np.uint8)
    if img.ndim != 2:
        raise NotImplementedError(f"skeletonize_host takes one 2-D image, got shape {img.shape}")
    removing = 0
    while img.size:
        removed = False
        for table in _TABLES:
            gone = table[_neighbour_code(img)] & (img != 0)
            if gone.any():
                img[gone] = 0
                removed = True
        if not removed:
            break
        removing += 1
    return (img, removing) if return_passes else img


def skeletonize_device(mask, return_passes=False):
    """mask: CUDA tensor [H, W] or [B, H, W] of any dtype (non-zero = foreground) -> uint8 0 / 1 of the same shape on the same device
    (csrc/skeleton.hip; the images of a batch are independent). With return_passes also the double passes the slowest image took,
    counting the last one, which removed nothing. Waits on the current stream once per 8 double passes (the convergence flags)."""
    from .. import _native
    if not mask.is_cuda:
        raise RuntimeError("skeletonize_device takes a CUDA tensor; skeletonize_host is the CPU restatement")
    if mask.dim() not in (2, 3):
        raise NotImplementedError(f"skeletonize_device takes [H, W] or [B, H, W], got shape {tuple(mask.shape)} "
                                  "(the reference's 3-D method='lee' skeleton is not implemented)")
    shape = mask.shape
    m = (mask.detach().reshape(-1, shape[-2], shape[-1]) != 0).to(torch.uint8).contiguous()
    out = torch.empty_like(m)
    passes = ctypes.c_int(0)
    if m.numel():
        with torch.cuda.device(m.device):
            _native.launch("octa_skeletonize", m.device, m, m.shape[0], m.shape[1], m.shape[2], out, ctypes.byref(passes))
    out = out.view(shape)
    return (out, passes.value) if return_passes else out


def skeletonize(mask):
    """Skeleton of a torch tensor on the device it lives on, as uint8 0 / 1: CUDA -> the kernel, CPU -> the numpy restatement."""
    if mask.is_cuda:
        return skeletonize_device(mask)
    m = mask.detach().numpy()
    if m.ndim == 2:
        return torch.from_numpy(skeletonize_host(m))
    if m.ndim == 3:
        return torch.from_numpy(np.stack([skeletonize_host(x) for x in m])) if len(m) else torch.zeros(m.shape, dtype=torch.uint8)
    raise NotImplementedError(f"skeletonize takes [H, W] or [B, H, W], got shape {tuple(m.shape)}")
