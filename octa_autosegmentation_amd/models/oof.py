"""Optimally Oriented Flux (OOF) vessel filter -- the classical baseline `General.model.name: oof` (configs/config_oof.yml,
reference models/oof.py) -- on the GPU through csrc/oof.hip: a hand-written batched complex-double FFT, the radial OOF
filters of radii 1..5 and a closed-form 2x2 eigen-analysis per pixel.

`OOF()(img)` follows the reference's calling convention: float32 [B,1,H,W] in [0, 1] -> float64 of the same shape in [0, 1]
(the reference asserts B = 1; here every image of a batch is filtered and normalised on its own). It has no parameters;
`eval()` / `train()` do nothing. The host helpers below (`radius_constants`, `frequency_grid`, `radial_filter`) restate the
filter the kernels evaluate; the CPU tests build a float64 torch pipeline from them."""
import math

import torch

from .. import _native

RADII = (1, 2, 3, 4, 5)      # reference: num_radii 5, spacing (1, 1) -> radii 1..5
SIGMA = 1.0                  # min(spacing)
EPSILON = 1e-12


def radius_constants(r: int):
    """Per-radius constants of the filter, in the reference's operation order: (normalization, circle length 2 pi r, pi^2 r).
    besselj(1.5, z) / eps^1.5 at z = 2 pi r eps is its small-argument series' leading term (z / 2)^1.5 / Gamma(2.5): the next
    term is ~1e-22 relative, and the closed form sqrt(2 / (pi z)) (sin z / z - cos z) cancels completely at this z."""
    circle = 2 * math.pi * r
    z = circle * EPSILON
    bessel = math.pow(z / 2, 1.5) / math.gamma(2.5) / math.pow(EPSILON, 1.5)
    base = r / math.sqrt(2 * r * SIGMA - SIGMA * SIGMA)
    volume = math.pi * float(r * r)
    normalization = volume / bessel / float(r * r) * base
    return normalization, circle, (math.pi * math.pi) * r


def frequency_grid(h: int, w: int, device=None):
    """x (fftfreq(h) along rows), y (fftfreq(w) along columns) as float64 [h, w], rho = sqrt(x^2 + y^2) + 1e-12, and the
    Hermitian-symmetrised x y: 0 on the Nyquist row (h even) and the Nyquist column (w even), except on their shared corner."""
    kx = torch.arange(h, dtype=torch.float64, device=device)
    ky = torch.arange(w, dtype=torch.float64, device=device)
    x = (torch.where(kx < h - h // 2, kx, kx - h) / h)[:, None].expand(h, w)
    y = (torch.where(ky < w - w // 2, ky, ky - w) / w)[None, :].expand(h, w)
    rho = torch.sqrt(x * x + y * y) + EPSILON
    nyq_row = torch.zeros(h, 1, dtype=torch.bool, device=device)
    nyq_col = torch.zeros(1, w, dtype=torch.bool, device=device)
    if h % 2 == 0:
        nyq_row[h // 2] = True
    if w % 2 == 0:
        nyq_col[0, w // 2] = True
    xy = torch.where(nyq_row ^ nyq_col, torch.zeros((), dtype=torch.float64, device=device), x * y)
    return x, y, rho, xy


def radial_filter(rho: torch.Tensor, r: int) -> torch.Tensor:
    """H_r(rho) of one radius (reference oof.py:75-83, the same operation order)."""
    normalization, circle, kb = radius_constants(r)
    num = normalization * torch.exp((-2.0 * (math.pi * math.pi)) * (rho * rho))
    den = torch.pow(rho, 1.5)
    cs = circle * rho
    a = torch.sin(cs) / cs - torch.cos(cs)
    b = torch.sqrt(1.0 / (kb * rho))
    return num / den * a * b


def _require_cuda(t: torch.Tensor, who: str):
    if not t.is_cuda:
        raise RuntimeError(f"{who} runs on the GPU (no CPU fallback): pass --General.device cuda:0")


def fft2_c2c_f64(x: torch.Tensor, inverse: bool = False) -> torch.Tensor:
    """complex128 CUDA [..., H, W] -> its 2-D DFT (numpy.fft.fft2), or with `inverse` numpy.fft.ifft2 (1 / (H W) included)."""
    _require_cuda(x, "fft2_c2c_f64")
    if x.dtype != torch.complex128:
        raise TypeError(f"fft2_c2c_f64 takes complex128, got {x.dtype}")
    h, w = x.shape[-2], x.shape[-1]
    xc = x.reshape(-1, h, w).contiguous()
    b = xc.shape[0]
    out = torch.empty_like(xc)
    with torch.cuda.device(x.device):
        ws = torch.empty(max(1, _native.lib().octa_fft2_c2c_f64_workspace_bytes(b, h, w)), dtype=torch.uint8, device=x.device)
        # these entry points take a stream but no context (they bring their workspace along): call(), with the stream as an argument
        _native.call("octa_fft2_c2c_f64", xc, out, b, h, w, int(bool(inverse)), ws, _native.current_stream_ptr())
    return out.view(x.shape)


def _oof_call(img: torch.Tensor, normalize: bool) -> torch.Tensor:
    _require_cuda(img, "OOF")
    if img.dtype != torch.float32:
        raise TypeError(f"OOF takes float32 images in [0, 1] (as the configs' CastToTyped gives them), got {img.dtype}")
    if img.dim() < 2:
        raise ValueError(f"OOF needs an image [..., H, W], got shape {tuple(img.shape)}")
    h, w = img.shape[-2], img.shape[-1]
    x = img.reshape(-1, h, w).contiguous()
    b = x.shape[0]
    out = torch.empty(x.shape, dtype=torch.float64, device=img.device)
    with torch.cuda.device(img.device):
        ws = torch.empty(max(1, _native.lib().octa_oof_workspace_bytes(b, h, w)), dtype=torch.uint8, device=img.device)
        _native.call("octa_oof_2d" if normalize else "octa_oof_2d_response", x, out, b, h, w, ws, _native.current_stream_ptr())
    return out.view(img.shape)


class OOF:
    """2-D Optimally Oriented Flux filter with the reference's fixed settings (radii 1..5, sigma 1, response_type 1,
    use_absolute, normalization_type 1). Binarisation is left to the post-processing chain."""

    def __init__(self, **kwargs) -> None:
        pass

    def __call__(self, img: torch.Tensor) -> torch.Tensor:
        """img: CUDA float32 [B,1,H,W] in [0, 1] -> float64 [B,1,H,W]: per image (R + M) / max(R + M), R the response, M = max R."""
        return _oof_call(img, normalize=True)

    def response(self, img: torch.Tensor) -> torch.Tensor:
        """The response R before the normalisation (the reference's OOF._compute_oof of img * 255), float64 of img.shape."""
        return _oof_call(img, normalize=False)

    def eval(self):
        return self

    def train(self, mode: bool = True):
        return self
