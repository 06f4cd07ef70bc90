"""Frangi vesselness filter -- the classical baseline `General.model.name: frangi` (configs/config_frangi.yml, reference
models/frangi.py: skimage.filters.frangi(img * 255, sigmas=(0.5, 2, 0.5), alpha=1, beta=15, black_ridges=False)) -- on the GPU
through csrc/frangi.hip: separable Gaussian-derivative Hessians in float32 with double accumulation in scipy's order, closed-form
eigenvalues, the vesselness with its per-image gamma.

`Frangi()(img)` follows the reference's calling convention: float32 [B,1,H,W] in [0, 1] -> float64 of the same shape (the
reference asserts B = 1; here every image of a batch is filtered on its own, with its own gamma). It has no parameters; `eval()`
/ `train()` do nothing.

The filter is discontinuous, so the Hessian and eigenvalues are bit-identical to scikit-image's float32 ones. That needs the 1-D
weight tables to the bit: `gaussian_weights` builds them with numpy exactly as scipy.ndimage does, and the four tables of the
reference's two scales are kept below as `float.hex` constants -- numpy's exp in double is not the same to the last bit on every
CPU, and the reference configuration must not depend on the host it runs on."""
import math

import numpy as np
import torch

from .. import _native
from .oof import _require_cuda

SIGMAS = (0.5, 2, 0.5)       # the reference's tuple of scales (not a range); the third repeats the first
BETA = 15
MAX_SCALES = 8


def scaled_sigma_and_radius(sigma):
    """sigma' = sigma / sqrt(2) and scipy's radius int(truncate sigma' + 0.5), truncate 8 for sigma > 1 and 100 otherwise
    (skimage's hessian_matrix with use_gaussian_derivatives)."""
    sp = (1 / math.sqrt(2)) * sigma
    truncate = 8 if sigma > 1 else 100
    return sp, int(truncate * sp + 0.5)


def _build_weights(sigma, order):
    sp, radius = scaled_sigma_and_radius(sigma)
    sigma2 = sp * sp
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / sigma2 * x ** 2)
    phi = phi / phi.sum()
    if order == 0:
        return phi
    return (0 + x * (1 / -sigma2)) * phi       # scipy's polynomial construction for order 1: q(x) = 0 + x (1 / -sigma'^2)


# The tables of the reference's scales, offsets 0 .. (last non-zero tap); the table is symmetric (order 0) or antisymmetric
# (order 1) to the bit and zero beyond. (sigma, order) -> hex values.
_HALF_TABLES = {
    (0.5, 0): (   # radius 35, non-zero up to offset 13
        "0x1.ede84d3dfe6cbp-1", "0x1.217ab78fc2f09p-6", "0x1.d24158fbe09b9p-24", "0x1.01f90c3055774p-52",
        "0x1.883eeda9e7dcep-93", "0x1.99bf76cfb4b44p-145", "0x1.2611aaf4933c3p-208", "0x1.21fdedd08347ep-283",
        "0x1.88f0b89ac367dp-370", "0x1.6dcc4d97a2cc1p-468", "0x1.d3e8664b99821p-578", "0x1.9b333ea6531eap-699",
        "0x1.f0891c207a491p-832", "0x1.9beda0fe57ccdp-976",
    ),
    (0.5, 1): (   # radius 35, non-zero up to offset 13
        "0x0.0p+0", "-0x1.217ab78fc2f0ap-3", "-0x1.d24158fbe09bbp-20", "-0x1.82f5924880330p-48", "-0x1.883eeda9e7dd0p-88",
        "-0x1.0017aa41d0f0bp-139", "-0x1.b91a806edcda7p-203", "-0x1.fb7c602ce5bdfp-278", "-0x1.88f0b89ac367fp-364",
        "-0x1.9b85d74a9725bp-462", "-0x1.24713fef3ff16p-571", "-0x1.1ab33b1259252p-692", "-0x1.7466d5185bb6fp-825",
        "-0x1.4eb112cea7568p-969",
    ),
    (2.0, 0): (   # radius 11, non-zero up to offset 11
        "0x1.20dd750429b6fp-2", "0x1.c1efca49a5014p-3", "0x1.a911f096fbc26p-4", "0x1.e723726b824a8p-6", "0x1.529b9e8cf9a1bp-8",
        "0x1.1d83170fbf6f4p-11", "0x1.2408e9ba33277p-15", "0x1.6a597219a93c5p-20", "0x1.10b1488aeb226p-25",
        "0x1.f1e3523b41d60p-32", "0x1.13af4f04f9977p-38", "0x1.7258610b3b207p-46",
    ),
    (2.0, 1): (   # radius 11, non-zero up to offset 11
        "0x0.0p+0", "-0x1.c1efca49a5016p-4", "-0x1.a911f096fbc28p-4", "-0x1.6d5a95d0a1b80p-5", "-0x1.529b9e8cf9a1cp-7",
        "-0x1.64e3dcd3af4b2p-10", "-0x1.b60d5e974cbb5p-14", "-0x1.3d0e43d67414ep-18", "-0x1.10b1488aeb227p-23",
        "-0x1.180fde4155087p-29", "-0x1.589b22c637fd6p-36", "-0x1.fd39856f714cbp-44",
    ),
}


def gaussian_weights(sigma, order):
    """scipy.ndimage's 1-D weight table (`_gaussian_kernel1d(sigma', order, R)`) of one scale: float64 [2 R + 1], offsets -R .. R.
    The reference's scales come from the module's constants, any other sigma is built with numpy at run time."""
    if order not in (0, 1):
        raise ValueError(f"order must be 0 or 1, got {order}")
    half = _HALF_TABLES.get((float(sigma), order))
    if half is None:
        return _build_weights(sigma, order)
    radius = scaled_sigma_and_radius(sigma)[1]
    w = np.zeros(2 * radius + 1, dtype=np.float64)
    if order == 1:
        w[radius:] = -0.0       # (k / -sigma'^2) * 0.0 for k > 0: scipy's zeros carry the sign, and so do these
    pos = np.array([float.fromhex(v) for v in half], dtype=np.float64)
    w[radius - len(pos) + 1:radius + 1] = (pos if order == 0 else -pos)[::-1]
    w[radius:radius + len(pos)] = pos
    return w


def _tables(sigma):
    """(radius, the order-0 table followed by the order-1 table) as the native entry points take one scale."""
    return scaled_sigma_and_radius(sigma)[1], np.ascontiguousarray(np.concatenate([gaussian_weights(sigma, 0), gaussian_weights(sigma, 1)]))


def _prepare(img, who):
    _require_cuda(img, who)
    if img.dtype != torch.float32:
        raise TypeError(f"{who} takes float32 images (as the configs' CastToTyped gives them), got {img.dtype}")
    if img.dim() < 2:
        raise ValueError(f"{who} needs an image [..., H, W], got shape {tuple(img.shape)}")
    h, w = img.shape[-2], img.shape[-1]
    x = img.reshape(-1, h, w).contiguous()
    return x, x.shape[0], h, w


def _workspace(b, h, w, n_scales, device):
    n = _native.lib().octa_frangi_workspace_bytes(b, h, w, n_scales)
    if n == 0:
        raise ValueError(f"Frangi: unsupported shape (need 1 <= H, W <= 4096, at most {MAX_SCALES} distinct scales): b={b} h={h} w={w} scales={n_scales}")
    return torch.empty(n, dtype=torch.uint8, device=device)


def frangi_2d(img255: torch.Tensor, sigmas=SIGMAS, beta=BETA, gamma=None, black_ridges=False, in_scale=1.0) -> torch.Tensor:
    """skimage.filters.frangi of 2-D images: CUDA float32 [..., H, W] (times `in_scale` in float32) -> float64 of the same shape.
    gamma None: per image max(s) / 2 of the first scale. A scale that repeats an earlier one gives the same planes and is skipped."""
    x, b, h, w = _prepare(img255, "Frangi")
    scales = list(dict.fromkeys(float(s) for s in sigmas))
    if not scales:
        raise ValueError("Frangi needs at least one scale")
    if gamma is not None and not gamma > 0:
        raise ValueError(f"gamma must be positive or None, got {gamma}")
    tabs = [_tables(s) for s in scales]
    radii = np.array([r for r, _ in tabs], dtype=np.int32)
    weights = np.ascontiguousarray(np.concatenate([t for _, t in tabs]))
    out = torch.empty(x.shape, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        ws = _workspace(b, h, w, len(scales), x.device)
        # these entry points take a stream but no context (they bring their workspace along): call(), with the stream as an argument
        _native.call("octa_frangi_2d", x, out, b, h, w, len(scales), radii.ctypes.data, weights.ctypes.data, float(in_scale), float(beta),
                     0.0 if gamma is None else float(gamma), int(bool(black_ridges)), ws, _native.current_stream_ptr())
    return out.view(img255.shape)


class Frangi:
    """2-D Frangi filter with the reference's fixed settings (sigmas (0.5, 2, 0.5), beta 15, bright ridges, gamma from the first
    scale). Binarisation is left to the post-processing chain."""

    def __init__(self, **kwargs) -> None:
        pass

    def __call__(self, img: torch.Tensor) -> torch.Tensor:
        """img: CUDA float32 [B,1,H,W] in [0, 1] -> float64 [B,1,H,W], the vesselness of img * 255 per image."""
        return frangi_2d(img, SIGMAS, BETA, None, False, in_scale=255.0)

    def _one_scale(self, img, sigma, entry, n_out):
        x, b, h, w = _prepare(img, "Frangi")
        radius, weights = _tables(sigma)
        outs = [torch.empty(x.shape, dtype=torch.float32, device=x.device) for _ in range(n_out)]
        gamma = [torch.empty(b, dtype=torch.float32, device=x.device)] if entry == "octa_frangi_eigenvalues" else []
        with torch.cuda.device(x.device):
            ws = _workspace(b, h, w, 1, x.device)
            _native.call(entry, x, *outs, *gamma, b, h, w, radius, weights.ctypes.data, 255.0, 0, ws, _native.current_stream_ptr())
        return [o.view(img.shape) for o in outs] + gamma

    def hessian(self, img: torch.Tensor, sigma):
        """(Hrr, Hrc, Hcc) of -(img * 255) at one scale, float32 of img.shape (skimage's hessian_matrix of the negated image)."""
        return tuple(self._one_scale(img, sigma, "octa_frangi_hessian", 3))

    def eigenvalues(self, img: torch.Tensor, sigma):
        """(lambda1, lambda2, gamma): that Hessian's eigenvalues sorted by magnitude, float32 of img.shape, and float32 [B] gamma =
        max(sqrt(lambda1^2 + lambda2^2)) / 2 per image (1 when 0) -- the filter's gamma when `sigma` is its first scale."""
        return tuple(self._one_scale(img, sigma, "octa_frangi_eigenvalues", 2))

    def eval(self):
        return self

    def train(self, mode: bool = True):
        return self
