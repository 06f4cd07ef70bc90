"""The training configs' augmentation chain on the GPU, for a whole batch that never leaves HBM.

Reference: `Train.data_augmentation` of configs/config_ves_seg-S.yml:28-102, instantiated by
data/data_transforms.py:587-611 (MONAI dictionary transforms on the CPU, one sample at a time in loader workers):
  LoadGraphAndFilterByRandomRadiusd -> ScaleIntensityd(0,1) -> EnsureChannelFirstd -> Resized(1216,1216, bilinear)
  -> RandFlipd(0.5, axes [0,1]) -> RandRotate90d(0.75) -> RandRotated(prob 1, +-range_x, zeros) -> AsDiscreted(label, 0.1)
  -> CastToTyped.
Here the rasteriser's uint8 batches (pipeline.TripleGenerator) go through two HIP kernels (csrc/augment.hip); the random
decisions are drawn on the host from one numpy RandomState in the order MONAI's `randomize` methods draw them
(flip: rand() < p; rot90: rand() < p, then randint(3) + 1; rotate: rand() < p, then uniform(-r, r)), image and label of a
sample share them. MONAI is not installed here: its per-transform random streams are not reproduced (parity unpinned),
the geometry is pinned against the torch ops MONAI delegates to (tests/test_augment_gpu.py).
The Giarratano set-up adds the reference's RandCropOrPadd behind RandRotated (configs/config_ves_seg-S_Giarratano.yml: 1216 -> 360): the
rotate kernel's window form computes the kept pixels only, bit for bit those of the full frame (tests/test_crop_gpu.py).
"""

import random as _py_random

import numpy as np
import torch

from .. import _native


def resize_bilinear(x, size, mul=None, add=None):
    """x: CUDA uint8 / float32 [B,h,w] -> float32 [B,H,W] (torch bilinear, align_corners=False); optional per-image
    affine map of the source values (ScaleIntensity)."""
    assert x.is_cuda and x.dim() == 3 and x.is_contiguous() and x.dtype in (torch.uint8, torch.float32)
    B, h, w = x.shape
    out = torch.empty((B, int(size[0]), int(size[1])), dtype=torch.float32, device=x.device)
    _native.launch("octa_resize_bilinear", x.device, x, 0 if x.dtype == torch.uint8 else 1, B, h, w, out, out.shape[1], out.shape[2], mul, add)
    return out


def resize_bilinear_bwd(dy, size):
    """Adjoint of resize_bilinear: dy CUDA float32 [B,H,W] -> float32 [B,h,w] with size = (h, w)."""
    assert dy.is_cuda and dy.dim() == 3 and dy.is_contiguous() and dy.dtype == torch.float32
    B, H, W = dy.shape
    dx = torch.empty((B, int(size[0]), int(size[1])), dtype=torch.float32, device=dy.device)
    _native.launch("octa_resize_bilinear_bwd", dy.device, dy, B, dx.shape[1], dx.shape[2], H, W, dx)
    return dx


class BilinearResize(torch.autograd.Function):
    """F.interpolate(x, size, mode="bilinear") (align_corners False) on [B, C, h, w] CUDA tensors through csrc/augment.hip, both ways."""

    @staticmethod
    def forward(ctx, x, size):
        B, C, h, w = x.shape
        ctx.in_shape, ctx.in_dtype = (h, w), x.dtype
        y = resize_bilinear(x.reshape(B * C, h, w).float().contiguous(), size)
        return y.view(B, C, int(size[0]), int(size[1])).to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        B, C, H, W = dy.shape
        dx = resize_bilinear_bwd(dy.reshape(B * C, H, W).float().contiguous(), ctx.in_shape)
        return dx.view(B, C, *ctx.in_shape).to(ctx.in_dtype), None


def flip_rot90_rotate(x, angle, rot_k=None, flip=None, threshold=None):
    """x: CUDA float32 [B,N,N]; angle float32 [B] (radians), rot_k / flip int32 [B] or None."""
    assert x.is_cuda and x.dim() == 3 and x.shape[1] == x.shape[2] and x.dtype == torch.float32 and x.is_contiguous()
    out = torch.empty_like(x)
    _native.launch("octa_flip_rot90_rotate", x.device, x, out, x.shape[0], x.shape[1], angle, rot_k, flip, float(threshold if threshold is not None else 0.0),
                   0 if threshold is None else 1)
    return out


def flip_rot90_rotate_window(x, angle, rot_k, flip, threshold, size, oy, ox):
    """The window [oy[b] : oy[b] + size[0], ox[b] : ox[b] + size[1]] of flip_rot90_rotate(x, angle, rot_k, flip, threshold), bit for bit, computed
    alone (RandCropOrPadd behind RandRotated): x CUDA float32 [B,N,N]; oy / ox int32 [B] on the device; what lies outside [0, N)^2 is 0
    before the threshold (negative offsets: the pad case). -> float32 [B, size[0], size[1]]."""
    assert x.is_cuda and x.dim() == 3 and x.shape[1] == x.shape[2] and x.dtype == torch.float32 and x.is_contiguous()
    for o in (oy, ox):
        assert o.is_cuda and o.dtype == torch.int32 and o.shape == (x.shape[0],) and o.is_contiguous()
    out = torch.empty((x.shape[0], int(size[0]), int(size[1])), dtype=torch.float32, device=x.device)
    _native.launch("octa_flip_rot90_rotate_window", x.device, x, out, x.shape[0], x.shape[1], angle, rot_k, flip,
                   float(threshold if threshold is not None else 0.0), 0 if threshold is None else 1, out.shape[1], out.shape[2], oy, ox)
    return out


def background_noise(img, noise, u, out_dtype=torch.float64):
    """AddRandomBackgroundNoised on device tensors of equal shape: img / noise float32, u float64 (numpy's uniform factors).
    Returns max(img, noise * u) as float64 (the reference's promoted dtype) or float32."""
    assert img.is_cuda and img.shape == noise.shape == u.shape and u.dtype == torch.float64
    img, noise, u = img.contiguous().float(), noise.contiguous().float(), u.contiguous()
    out = torch.empty(img.shape, dtype=out_dtype, device=img.device)
    o64, o32 = (out, None) if out_dtype == torch.float64 else (None, out)
    _native.launch("octa_background_noise", img.device, img, noise, u, img.numel(), o64, o32)
    return out


def speckle_brightness(img, grid9, u):
    """SpeckleBrightnesd on a device batch: img float32 [B,H,W], grid9 float32 [B,9,9] (control values in [0.5, 1)), u float32 [B,H,W]."""
    assert img.is_cuda and img.dim() == 3 and grid9.shape == (img.shape[0], 9, 9) and u.shape == img.shape
    img, grid9, u = img.contiguous().float(), grid9.contiguous().float(), u.contiguous().float()
    out = torch.empty_like(img)
    mm = torch.empty((img.shape[0], 2), dtype=torch.int32, device=img.device)
    _native.launch("octa_speckle_brightness", img.device, img, grid9, u, img.shape[0], img.shape[1], img.shape[2], out, mm)
    return out


class GpuSegAugmentation:
    """Batched replacement of the `data_augmentation` list of a segmentation config (the entries after the graph loader)."""

    def __init__(self, aug_config, seed=None):
        self.size, self.flip_p, self.rot90_p, self.rot_p, self.rot_range, self.threshold = None, 0.0, 0.0, 0.0, 0.0, None
        self.scale = None
        self.crop = None                 # RandCropOrPadd: (prob, min_factor, max_factor)
        for d in aug_config:
            name = d["name"]
            if name in ("LoadGraphAndFilterByRandomRadiusd", "EnsureChannelFirstd", "CastToTyped"):
                continue
            if name == "ScaleIntensityd":
                self.scale = (float(d.get("minv", 0.0)), float(d.get("maxv", 1.0)))
            elif name == "Resized":
                if d.get("mode", "bilinear") != "bilinear":
                    raise NotImplementedError("Resized: only mode bilinear is on the GPU path")
                self.size = [int(v) for v in d["spatial_size"]]
            elif name == "RandFlipd":
                if sorted(d.get("spatial_axis", [0, 1])) != [0, 1]:
                    raise NotImplementedError("RandFlipd: the configs flip both axes")
                self.flip_p = float(d.get("prob", 0.1))
            elif name == "RandRotate90d":
                self.rot90_p = float(d.get("prob", 0.1))
            elif name == "RandRotated":
                if d.get("padding_mode", "border") != "zeros":
                    raise NotImplementedError("RandRotated: only padding_mode zeros is on the GPU path")
                self.rot_p, self.rot_range = float(d.get("prob", 0.1)), float(d.get("range_x", 0.0))
            elif name == "AsDiscreted":
                self.threshold = float(d["threshold"])
            elif name == "RandCropOrPadd":
                if self.crop is not None:
                    raise NotImplementedError("RandCropOrPadd: the GPU augmentation chain takes one entry")
                self.crop = (d.get("prob", 0.1), d.get("min_factor", 1), d.get("max_factor", 1))
            else:
                raise NotImplementedError(f"transform {name} is not part of the GPU augmentation chain")
        # one generator PER random transform, all seeded alike -- what get_data_augmentations does with MONAI's Randomizable objects
        # (data_transforms.py:606-607) and what data/data_transforms.py's RandFlipd / RandRotate90d / RandRotated do: the fused chain
        # and the generic per-sample transforms take the same decisions for the same seed (tests/test_training_cli_gpu.py)
        self.R_flip, self.R_rot90, self.R_rot = (np.random.RandomState(seed) for _ in range(3))

    def draw(self, batch):
        """Per-sample (flip, k, angle), every transform drawing from its own stream in the order its `randomize` draws."""
        flip = np.zeros(batch, np.int32)
        k = np.zeros(batch, np.int32)
        ang = np.zeros(batch, np.float32)
        for b in range(batch):
            flip[b] = self.R_flip.rand() < self.flip_p
            kk = self.R_rot90.randint(3) + 1
            if self.R_rot90.rand() < self.rot90_p:
                k[b] = kk
            if self.R_rot.rand() < self.rot_p:
                ang[b] = self.R_rot.uniform(low=-self.rot_range, high=self.rot_range)
                self.R_rot.uniform(low=0.0, high=0.0)
                self.R_rot.uniform(low=0.0, high=0.0)
        return flip, k, ang

    def draw_crop(self, shape):
        """RandCropOrPadd's draws for ONE sample whose first key has the spatial `shape`, from the global `random` in the transform's order
        (data_transforms.RandCropOrPadd). -> (out_h, out_w, oy, ox): the window of the rotated frame; a pad is a window with negative offsets;
        not applied / factor 1 is the whole frame."""
        prob, lo, hi = self.crop
        H, W = int(shape[0]), int(shape[1])
        if not _py_random.uniform(0, 1) < prob:
            return H, W, 0, 0
        factor = _py_random.uniform(lo, hi)
        if factor < 1:
            s_x, s_y = int(H * factor), int(W * factor)
            oy = _py_random.randint(0, H - s_x)
            ox = _py_random.randint(0, W - s_y)
            return s_x, s_y, oy, ox
        if factor > 1:
            s_x, s_y = int(H * factor), int(W * factor)
            return s_x, s_y, -((s_x - H) // 2), -((s_y - W) // 2)
        return H, W, 0, 0

    def _scale_map(self, x):
        if self.scale is None:
            return None, None
        # per-sample extrema in two passes (rows first): a reduction of [B, h*w] to B values runs on B workgroups -- 0.37 ms per call for
        # four 1216^2 labels, 1.5 ms of reductions per training step on the loader's stream -- and the uint8 label needs no fp32 copy
        rows = x.reshape(x.shape[0], -1, x.shape[-1]) if x.dim() >= 3 else x.reshape(x.shape[0], 1, -1)
        mn, mx = rows.amin(dim=2).amin(dim=1).float(), rows.amax(dim=2).amax(dim=1).float()
        lo, hi = self.scale
        span = mx - mn
        mul = torch.where(span > 0, (hi - lo) / span, torch.zeros_like(span))     # MONAI: a constant image maps to minv
        return mul.contiguous(), (lo - mn * mul).contiguous()

    def __call__(self, image, label, windows=None):
        """image, label: CUDA uint8 / float32 [B,h,w] (rasteriser output). -> dict(image, label) float32 [B,1,H,W]. With a RandCropOrPadd entry
        only the windows are computed (octa_flip_rot90_rotate_window): `windows` = one draw_crop() result per sample, all of one size (None:
        drawn here, sample by sample) -> [B,1,out_h,out_w], the offsets in params["crop_oy"] / ["crop_ox"]."""
        B = image.shape[0]
        flip, k, ang = self.draw(B)
        dev = image.device
        flip_t, k_t, ang_t = (torch.from_numpy(a).to(dev) for a in (flip, k, ang))
        params = dict(flip=flip, rot_k=k, angle=ang)
        if self.crop is not None:
            frame = self.size or list(image.shape[1:])           # the first key's shape after Resized: RandCropOrPadd takes its slices from it
            if (self.size or list(label.shape[1:])) != frame:
                raise NotImplementedError("RandCropOrPadd on the GPU augmentation chain: image and label need one size in front of the crop")
            if windows is None:
                windows = [self.draw_crop(frame) for _ in range(B)]
            if len(windows) != B or len({tuple(w[:2]) for w in windows}) != 1:
                raise ValueError(f"RandCropOrPadd: a mini-batch is stacked from windows of one size, got {sorted({tuple(w[:2]) for w in windows})}")
            oy, ox = (np.array([w[i] for w in windows], dtype=np.int32) for i in (2, 3))
            oy_t, ox_t = torch.from_numpy(oy).to(dev), torch.from_numpy(ox).to(dev)
            params.update(crop_oy=oy, crop_ox=ox)
        out = {}
        for key, x, thr in (("image", image, None), ("label", label, self.threshold)):
            mul, add = self._scale_map(x)
            size = self.size or list(x.shape[1:])
            y = resize_bilinear(x.contiguous(), size, mul, add)
            if self.crop is None:
                out[key] = flip_rot90_rotate(y, ang_t, k_t, flip_t, thr).unsqueeze(1)
            else:
                out[key] = flip_rot90_rotate_window(y, ang_t, k_t, flip_t, thr, windows[0][:2], oy_t, ox_t).unsqueeze(1)
        out["params"] = params
        return out


# ---- the Menten et al. augmentation (csrc/menten.hip; draws and host restatement: data/menten.py) ------------------------------------

_MENTEN_WEIGHTS = {}


def _gauss_weights(sigma, device):
    """scipy's Gaussian taps for `sigma` as a float64 device tensor, computed on the host once per (sigma, device)."""
    from . import menten
    key = (float(sigma), str(device))
    if key not in _MENTEN_WEIGHTS:
        _MENTEN_WEIGHTS[key] = torch.from_numpy(menten.gaussian_weights(sigma)).to(device)
    return _MENTEN_WEIGHTS[key]


def menten_vessel_noise(img, bernoulli, quantum, sigma=1.0, scaling=0.5, r=48):
    """BinomialVesselNoised on a device batch: img float32 / float64 [B,H,W], bernoulli uint8 [B,H,W] (np.random.binomial(1, 0.1)), quantum
    float64 [B,H,W] (np.random.uniform(0, 0.2)). -> float64 [B,H,W]."""
    assert img.is_cuda and img.dim() == 3 and img.dtype in (torch.float32, torch.float64)
    assert bernoulli.shape == img.shape and bernoulli.dtype == torch.uint8 and quantum.shape == img.shape and quantum.dtype == torch.float64
    img, bernoulli, quantum = img.contiguous(), bernoulli.contiguous(), quantum.contiguous()
    w = _gauss_weights(sigma, img.device)
    B, H, W = img.shape
    tmp = torch.empty((B, H, W), dtype=torch.float64, device=img.device)
    out = torch.empty_like(tmp)
    _native.launch("octa_menten_vessel_noise", img.device, img, 0 if img.dtype == torch.float32 else 1, bernoulli, quantum, w, (w.numel() - 1) // 2,
                   float(scaling), float(r), B, H, W, tmp, out)
    return out


def _floater_args(points, dilations, device):
    """[int array [n_b + 1, 2]] per sample, [int] -> device int32 tensors pts [B,P,2], npts [B], dil [B]."""
    P = max(len(p) for p in points)
    pts = np.zeros((len(points), P, 2), dtype=np.int32)
    for b, p in enumerate(points):
        pts[b, :len(p)] = np.asarray(p, dtype=np.int32).reshape(-1, 2)
    npts = np.array([len(p) for p in points], dtype=np.int32)
    dil = np.asarray(dilations, dtype=np.int32).reshape(len(points))
    return tuple(torch.from_numpy(a).to(device) for a in (pts, npts, dil)) + (P,)


def menten_floater_mask(points, dilations, N, device):
    """The boolean mask of AddVitreousFloater alone, binary_dilation(lines, iterations=dilations), for B samples: points[b] int [n_b + 1, 2] (the
    corners of the walk, indices along the mask's (first, second) axis), dilations[b] >= 1. -> bool [B,N,N] on `device`."""
    pts, npts, dil, P = _floater_args(points, dilations, device)
    B = pts.shape[0]
    mask = torch.empty((B, N, N), dtype=torch.uint8, device=device)
    dist = torch.empty((B, N, N), dtype=torch.int32, device=device)
    _native.launch("octa_menten_floater_mask", mask.device, pts, npts, dil, B, P, N, mask, dist)
    return mask.bool()


def menten_floater(img, points, dilations, sigma=10):
    """AddVitreousFloater on a device batch of SQUARE float64 images [B,N,N] that all get a floater: img * (1 - gaussian_filter(mask, sigma)) with
    the mask of menten_floater_mask. -> float64 [B,N,N]."""
    assert img.is_cuda and img.dim() == 3 and img.shape[1] == img.shape[2] and img.dtype == torch.float64 and len(points) == img.shape[0]
    img = img.contiguous()
    B, N, _ = img.shape
    pts, npts, dil, P = _floater_args(points, dilations, img.device)
    w = _gauss_weights(sigma, img.device)
    mask = torch.empty((B, N, N), dtype=torch.uint8, device=img.device)
    dist = torch.empty((B, N, N), dtype=torch.int32, device=img.device)
    tmp = torch.empty_like(img)
    out = torch.empty_like(img)
    _native.launch("octa_menten_floater", img.device, img, pts, npts, dil, w, (w.numel() - 1) // 2, B, P, N, mask, dist, tmp, out)
    return out


def menten_motion(x, table, white=None):
    """AddMotionArtifact's cuts as one gather (data/menten.py fold_cuts): x [B,H,W] of a 4- or 8-byte dtype, table int32 numpy [B,H,2] or [H,2]
    (source row, shift), white float64 numpy [k,W] (whiteout rows, cast to x's dtype as numpy's assignment does) or None. -> new tensor like x."""
    assert x.is_cuda and x.dim() == 3 and x.element_size() in (4, 8)
    x = x.contiguous()
    B, H, W = x.shape
    table = np.ascontiguousarray(np.asarray(table, dtype=np.int32).reshape(B, H, 2))
    esz = x.element_size()
    unit = 16 // esz                                     # 16-byte accesses where the row length and every shift allow it
    while unit > 1 and (W % unit or np.any(table[..., 1] % unit) or x.data_ptr() % (unit * esz)):
        unit //= 2
    d_white, n_white = None, 0
    if white is not None:
        np_dtype = torch.empty((), dtype=x.dtype).numpy().dtype
        d_white = torch.from_numpy(np.ascontiguousarray(np.asarray(white).astype(np_dtype))).to(x.device)
        n_white = d_white.shape[0]
        assert d_white.shape[1] == W
    d_table = torch.from_numpy(table).to(x.device)
    out = torch.empty_like(x)
    _native.launch("octa_menten_motion", x.device, x, out, esz, d_table, d_white, n_white, unit, B, H, W)
    return out


# ---- the reference's noise model (csrc/noise_model.hip; control-point draws and host restatement: data/noise_model.py) --------------------------

def noise_model(img, background, grids, seed, lambda_delta=1, lambda_speckle=0.7, lambda_gamma=0.3, delta=None, n=None, return_fields=False,
                sample_offset=0):
    """NoiseModeld's arithmetic AND its per-pixel Beta draws for a device batch in one launch: img, background float32 [B,H,W]; grids float32
    [B,5,gh,gw] (alpha_v, beta_v, alpha_s, beta_s, gamma control points, data/noise_model.py); seed: the 64-bit key of the call's counter-based
    generator, sample b draws under sample counter sample_offset + b. delta / n (float32 [B,H,W]) replace the drawn Delta / N field.
    -> float32 [B,H,W]; with return_fields (out, maps [B,5,H,W] -- the four clamped shape maps and Gamma --, fields [B,2,H,W] -- Delta, N)."""
    assert img.is_cuda and img.dim() == 3 and img.dtype == torch.float32 and background.shape == img.shape and background.dtype == torch.float32
    assert grids.dim() == 4 and grids.shape[:2] == (img.shape[0], 5) and grids.dtype == torch.float32
    dev = img.device
    img, background, grids = img.contiguous(), background.to(dev).contiguous(), grids.to(dev).contiguous()
    B, H, W = img.shape
    for f in (delta, n):
        assert f is None or (f.is_cuda and f.shape == img.shape and f.dtype == torch.float32)
    delta, n = (f.contiguous() if f is not None else None for f in (delta, n))
    out = torch.empty_like(img)
    maps = torch.empty((B, 5, H, W), dtype=torch.float32, device=dev) if return_fields else None
    fields = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev) if return_fields else None
    _native.launch("octa_noise_model", dev, img, background, grids, B, H, W, grids.shape[2], grids.shape[3], int(seed) & 0xFFFFFFFFFFFFFFFF,
                   int(sample_offset) & 0xFFFFFFFF, float(lambda_delta), float(lambda_speckle), float(lambda_gamma), delta, n, out, maps, fields)
    return (out, maps, fields) if return_fields else out


def noise_model_backward(dout, img, background, grids, seed, lambda_delta=1, lambda_speckle=0.7, lambda_gamma=0.3, delta=None, n=None,
                         return_intermediates=False, sample_offset=0):
    """The gradient of sum(noise_model(...) * dout) with respect to `grids` (csrc/noise_model.hip, octa_noise_model_backward): the arguments
    after dout are the forward call's; Delta and N are regenerated from the seed, nothing is kept from the forward. Deterministic, no atomics.
    -> dgrids float32 [B,5,gh,gw]; with return_intermediates (dgrids, {"dmaps" [B,5,H,W] the gradient with respect to the five maps, "out"
    [B,H,W] the re-run forward's output, "maps" [B,5,H,W], "logodds" [B,2,H,W] t = log(x / (1 - x)) of Delta and N, "bgrad" [B,4,H,W]
    dDelta/dalpha_v, dDelta/dbeta_v, dN/dalpha_s, dN/dbeta_s})."""
    assert img.is_cuda and img.dim() == 3 and img.dtype == torch.float32 and background.shape == img.shape and background.dtype == torch.float32
    assert grids.dim() == 4 and grids.shape[:2] == (img.shape[0], 5) and grids.dtype == torch.float32
    assert dout.shape == img.shape and dout.dtype == torch.float32 and dout.device == img.device
    dev = img.device
    dout, img, background, grids = dout.contiguous(), img.contiguous(), background.to(dev).contiguous(), grids.detach().to(dev).contiguous()
    B, H, W = img.shape
    for f in (delta, n):
        assert f is None or (f.is_cuda and f.shape == img.shape and f.dtype == torch.float32)
    delta, n = (f.contiguous() if f is not None else None for f in (delta, n))
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    dgrids, dmaps = torch.empty_like(grids), new(B, 5, H, W)
    extra = {"out": new(B, H, W), "maps": new(B, 5, H, W), "logodds": new(B, 2, H, W), "bgrad": new(B, 4, H, W)} if return_intermediates else {}
    _native.launch("octa_noise_model_backward", dev, dout, img, background, grids, B, H, W, grids.shape[2], grids.shape[3], int(seed) & 0xFFFFFFFFFFFFFFFF,
                   int(sample_offset) & 0xFFFFFFFF, float(lambda_delta), float(lambda_speckle), float(lambda_gamma), delta, n, dgrids, dmaps, extra.get("out"),
                   extra.get("maps"), extra.get("logodds"), extra.get("bgrad"))
    return (dgrids, dict(extra, dmaps=dmaps)) if return_intermediates else dgrids


class _NoiseModelRsample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids, img, background, seed, lambdas, delta, n, sample_offset):
        ctx.save_for_backward(grids, img, background, delta, n)
        ctx.call = (seed, lambdas, sample_offset)
        return noise_model(img, background, grids.detach(), seed, *lambdas, delta=delta, n=n, sample_offset=sample_offset)

    @staticmethod
    def backward(ctx, dout):
        grids, img, background, delta, n = ctx.saved_tensors
        seed, lambdas, sample_offset = ctx.call
        dgrids = noise_model_backward(dout.float().contiguous(), img, background, grids, seed, *lambdas, delta=delta, n=n, sample_offset=sample_offset)
        return dgrids, None, None, None, None, None, None, None


def noise_model_rsample(img, background, grids, seed, lambda_delta=1, lambda_speckle=0.7, lambda_gamma=0.3, delta=None, n=None, sample_offset=0):
    """noise_model(...) as a differentiable function of `grids` (the reference's NoiseModel.forward with Beta.rsample): forward the
    octa_noise_model launch, backward octa_noise_model_backward, which redraws Delta and N from the seed. The gradient goes to `grids` only.
    img, background: float32 [B,H,W] on the device, without gradient; grids float32 [B,5,gh,gw] on the same device."""
    assert not (img.requires_grad or background.requires_grad), "noise_model_rsample differentiates with respect to the control grids only"
    assert grids.is_cuda and grids.device == img.device
    return _NoiseModelRsample.apply(grids, img, background, int(seed), (float(lambda_delta), float(lambda_speckle), float(lambda_gamma)), delta, n,
                                    int(sample_offset))
