"""SkrGAN sketch filter -- the classical baseline `General.model.name: skrgan` (configs/config_skrgan.yml, reference
models/skrgan.py: Sobel magnitude, Gaussian low pass, skimage.morphology.area_opening and area_closing, each stage min/max
normalised) -- on the GPU through csrc/morph.hip: scipy's separable passes to the bit, and a grey-level area opening evaluated
per seed in registers.

`SkrGAN()(img)` follows the reference's calling convention: float32 [B,1,H,W] -> float32 of the same shape (the reference squeezes
the tensor to one 2-D image; here every image of a batch is filtered and normalised on its own). Like the reference's, the
constructor stores the area thresholds and connectivities and the call ignores them: it passes `sigma` and the hard-coded 64 / 64.
`sketch_filter` honours its arguments. An image with a constant stage is NaN everywhere, as numpy's 0 / 0 makes it.

The Gaussian needs scipy's 1-D weight table to the bit: `gaussian_weights` builds it with numpy exactly as scipy.ndimage does, and
the table of the reference's sigma = 2 is kept below as `float.hex` constants -- numpy's exp in double is not the same to the last
bit on every CPU, and the reference configuration must not depend on the host it runs on (models/frangi.py does the same)."""
import numpy as np
import torch

from .. import _native
from .oof import _require_cuda

SIGMA = 2
AREA_THRESHOLD = 64          # hard-coded in the reference's call, whatever the constructor was given
MAX_AREA = 128
TRUNCATE = 4.0               # scipy.ndimage.gaussian_filter's default

# scipy's table of sigma = 2 (radius 8), offsets 0 .. 8; it is symmetric to the bit
_HALF_TABLE_SIGMA_2 = (
    "0x1.98862a07ae7b4p-3", "0x1.68856f9ab1982p-3", "0x1.ef9093fc46e5ap-4", "0x1.0941b71ceef37p-4", "0x1.ba4d4125ffd2ap-6",
    "0x1.1f30504e20207p-7", "0x1.227362b5fc92dp-9", "0x1.c98b8c5d0dda5p-12", "0x1.18aad19e4159bp-14",
)


def gaussian_radius(sigma):
    """scipy's radius int(truncate sigma + 0.5) with the default truncate 4."""
    return int(TRUNCATE * float(sigma) + 0.5)


def _build_weights(sigma):
    sigma = float(sigma)
    radius = gaussian_radius(sigma)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def gaussian_weights(sigma):
    """scipy.ndimage's 1-D weight table `_gaussian_kernel1d(sigma, 0, R)`: float64 [2 R + 1], offsets -R .. R. The reference's sigma
    comes from the module's constants, any other is built with numpy at run time. None for sigma <= 1e-15: scipy copies the input."""
    if float(sigma) <= 1e-15:
        return None
    if float(sigma) != 2.0:
        return _build_weights(sigma)
    pos = np.array([float.fromhex(v) for v in _HALF_TABLE_SIGMA_2], dtype=np.float64)
    return np.concatenate([pos[:0:-1], pos])


def _prepare(img, who):
    _require_cuda(img, who)
    if img.dtype != torch.float32:
        raise TypeError(f"{who} takes float32 images (as the configs' CastToTyped gives them), got {img.dtype}")
    if img.dim() < 2:
        raise ValueError(f"{who} needs an image [..., H, W], got shape {tuple(img.shape)}")
    h, w = img.shape[-2], img.shape[-1]
    x = img.reshape(-1, h, w).contiguous()
    return x, x.shape[0], h, w


def _check_area(area_threshold, connectivity, h, w, who):
    if connectivity != 1:
        raise ValueError(f"{who}: only connectivity 1 (4 neighbours) is built, got {connectivity}")
    if int(area_threshold) != area_threshold or not 1 <= area_threshold <= MAX_AREA:
        raise ValueError(f"{who}: the area threshold must be an integer in 1 .. {MAX_AREA}, got {area_threshold}")
    if h * w < area_threshold:
        raise ValueError(f"{who}: an image of {h} x {w} pixels has fewer than the area threshold {area_threshold}")
    return int(area_threshold)


def _workspace(b, h, w, device, who):
    n = _native.lib().octa_skr_workspace_bytes(b, h, w)
    if n == 0:
        raise ValueError(f"{who}: unsupported shape (need 1 <= H, W <= 4096, B <= 65535): b={b} h={h} w={w}")
    return torch.empty(n, dtype=torch.uint8, device=device)


def _open(img, area_threshold, connectivity, closing, who):
    if img.dim() >= 2:
        area_threshold = _check_area(area_threshold, connectivity, img.shape[-2], img.shape[-1], who)
    x, b, h, w = _prepare(img, who)
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        ws = _workspace(b, h, w, x.device, who) if closing else None
        _native.call("octa_area_opening", x, out, b, h, w, area_threshold, int(closing), ws, _native.current_stream_ptr())
    return out.view(img.shape)


def area_opening(img: torch.Tensor, area_threshold=64, connectivity=1) -> torch.Tensor:
    """skimage.morphology.area_opening of 2-D images: CUDA float32 [..., H, W] -> the same shape. Every bright 4-connected
    component of fewer than `area_threshold` pixels is lowered to the highest level at which it has that many."""
    return _open(img, area_threshold, connectivity, False, "area_opening")


def area_closing(img: torch.Tensor, area_threshold=64, connectivity=1) -> torch.Tensor:
    """skimage.morphology.area_closing as recalled: invert (1 - x in float32), open, invert."""
    return _open(img, area_threshold, connectivity, True, "area_closing")


def sketch_stages(img: torch.Tensor, sigma=SIGMA, area_open=AREA_THRESHOLD, area_close=AREA_THRESHOLD):
    """(normalised Sobel magnitude, Gaussian-filtered plane, normalised opened plane, output), each float32 of img.shape."""
    who = "SkrGAN"
    if img.dim() >= 2:
        area_open = _check_area(area_open, 1, img.shape[-2], img.shape[-1], who)
        area_close = _check_area(area_close, 1, img.shape[-2], img.shape[-1], who)
    x, b, h, w = _prepare(img, who)
    if float(sigma) < 0:
        raise ValueError(f"sigma must not be negative, got {sigma}")
    weights = gaussian_weights(sigma)
    radius = -1 if weights is None else len(weights) // 2
    weights = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    planes = [torch.empty_like(x) for _ in range(4)]
    with torch.cuda.device(x.device):
        ws = _workspace(b, h, w, x.device, who)
        _native.call("octa_skr_filter", x, *planes, b, h, w, radius, None if weights is None else weights.ctypes.data, area_open, area_close, ws,
                     _native.current_stream_ptr())
    return tuple(p.view(img.shape) for p in planes)


def sketch_filter(img: torch.Tensor, sigma=SIGMA, area_open=AREA_THRESHOLD, area_close=AREA_THRESHOLD) -> torch.Tensor:
    """The reference's filter with its three numbers as arguments: CUDA float32 [..., H, W] -> float32 of the same shape."""
    return sketch_stages(img, sigma, area_open, area_close)[3]


class SkrGAN:
    """The sketch filter with the reference's constructor and its quirk: the thresholds and connectivities are stored and ignored."""

    def __init__(self, sigma=2, area_threshold_open=64, connectivity_open=1, area_threshold_close=64, connectivity_close=1) -> None:
        self.sigma = sigma
        self.area_threshold_open = area_threshold_open
        self.connectivity_open = connectivity_open
        self.area_threshold_close = area_threshold_close
        self.connectivity_close = connectivity_close

    def __call__(self, img: torch.Tensor) -> torch.Tensor:
        """img: CUDA float32 [B,1,H,W] -> float32 [B,1,H,W], each image filtered on its own."""
        return sketch_filter(img, self.sigma, AREA_THRESHOLD, AREA_THRESHOLD)

    def stages(self, img: torch.Tensor):
        """The four planes of the call: normalised magnitude, filtered, normalised opened, output."""
        return sketch_stages(img, self.sigma, AREA_THRESHOLD, AREA_THRESHOLD)

    def eval(self):
        return self

    def train(self, mode: bool = True):
        return self
