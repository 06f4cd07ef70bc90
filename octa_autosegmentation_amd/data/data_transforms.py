"""Dictionary transforms of the training / validation / test configs, without MONAI (reference data/data_transforms.py;
registry :587-611). Every transform keeps its YAML name and constructor arguments and is a callable dict -> dict, so the
reference's config lists drive them unchanged. Tensors live on the GPU from the moment they are loaded: samples are
transformed where they will be consumed instead of in CPU loader workers.

Two groups:
* the reference's OWN transforms on the hot path -- LoadGraphAndFilterByRandomRadiusd (:358-387), ToGrayScaled (:389-400),
  SpeckleBrightnesd (:25-42), AddRandomBackgroundNoised (:498-516), ImageToImageTranslationd (:327-356), and the comparison baseline
  MentenAugmentationd with its parts BinomialVesselNoised, AddVitreousFloater, AddMotionArtifact (:44-325), and the paper's own noise
  model NoiseModeld with RandomDecreaseResolutiond (:435-496), and RandCropOrPadd (:543-585), the random crop of the Giarratano set-up;
* the MONAI transforms those configs name (LoadImaged, ScaleIntensityd, EnsureChannelFirstd, Resized, RandFlipd, RandRotate90d,
  RandRotated, Rotate90d, Flipd, AsDiscreted, CastToTyped; post-processing: Activations, AsDiscrete, RemoveSmallObjects,
  KeepLargestConnectedComponent, CastToType; RemoveOuterNoise is the reference's own, :418-432), restated from MONAI's documented behaviour. MONAI is neither in the image nor under /root/reference:
  parity with MONAI itself -- in particular its per-transform random streams -- is UNPINNED; the geometry is pinned against
  the torch ops MONAI delegates to (tests/test_augment_gpu.py, tests/test_data_pipeline.py).
"""
import csv
import pickle
import random as _py_random

import numpy as np
import torch

from .._native import advance_python_random
from ..vessel_graph_generation import tree2img
from ..vessel_graph_generation.tree2img import rasterize_forest


_GRAPH_CACHE = {}          # (path, mtime, size) -> (edges float64 [n,7] on the host, the same on the device)
_GRAPH_CACHE_MAX = 4096


def load_graph_cached(path):
    """A graph CSV parsed once per process (native reader) and kept on the device: an epoch of the training loop re-reads every
    file (the reference parses 1.2 MB of text per sample and epoch in its loader workers)."""
    import os
    from .. import graph_io
    st = os.stat(path)
    key = (path, st.st_mtime_ns, st.st_size)
    hit = _GRAPH_CACHE.get(key)
    if hit is None:
        e = graph_io.read_csv_native(path)
        hit = (e, torch.from_numpy(e).to(default_device()))
        if len(_GRAPH_CACHE) >= _GRAPH_CACHE_MAX:
            _GRAPH_CACHE.pop(next(iter(_GRAPH_CACHE)))
        _GRAPH_CACHE[key] = hit
    return hit


def _as_keys(keys):
    return [keys] if isinstance(keys, str) else list(keys)


def default_device():
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")


class MapTransform:
    """dict -> dict transform over `keys` (MONAI's MapTransform convention: a missing key is an error unless
    allow_missing_keys)."""

    def __init__(self, keys, allow_missing_keys: bool = False):
        self.keys = _as_keys(keys)
        self.allow_missing_keys = allow_missing_keys

    def present(self, data):
        for k in self.keys:
            if k in data:
                yield k
            elif not self.allow_missing_keys:
                raise KeyError(f"{type(self).__name__}: key {k!r} is missing from the sample ({sorted(data)})")


class Randomizable:
    """Owns a numpy RandomState `R`; `set_random_state(seed)` as in MONAI (get_data_augmentations seeds every random
    transform with General.seed, data_transforms.py:606-607)."""

    R = np.random.RandomState()

    def set_random_state(self, seed=None, state=None):
        self.R = state if state is not None else np.random.RandomState(seed)
        return self


class Compose:
    def __init__(self, transforms=None):
        self.transforms = list(transforms or [])

    def __call__(self, data):
        for t in self.transforms:
            data = t(data)
        return data

    def batchable(self, has_background=True):
        """True when the chain holds a transform with a mini-batch form (`batch_apply`: the frozen generator of
        ImageToImageTranslationd) and may be cut there without changing any random decision. "All prefixes, one batched call, all
        suffixes" runs sample 2's prefix BEFORE sample 1's suffix, so it consumes every SHARED random stream in the per-sample
        order only if no such stream is drawn from on both sides of the cut. Every transform declares its streams
        (`rng_streams(has_background)`: "python" = the global `random`, "numpy" = numpy's global stream, "torch" = torch's global
        generator; a transform's own RandomState is private and never conflicts); a transform that declares nothing counts as
        deterministic only if it is not Randomizable and has no `R` -- an undeclared Randomizable that was never seeded still draws from
        the CLASS-level `Randomizable.R`, which every unseeded instance shares: that is a shared stream ("class_R")."""
        cut = [i for i, t in enumerate(self.transforms) if hasattr(t, "batch_apply")]
        if len(cut) != 1:
            return False

        def streams(ts):
            out = set()
            for t in ts:
                f = getattr(t, "rng_streams", None)
                if f is not None:
                    out |= set(f(has_background))
                elif isinstance(t, Randomizable) or hasattr(t, "R"):
                    if getattr(t, "R", None) is Randomizable.R:      # never seeded: the class-level RandomState all unseeded instances share
                        out.add("class_R")
            return out

        return not (streams(self.transforms[:cut[0]]) & streams(self.transforms[cut[0] + 1:]))

    def call_batch(self, items):
        """[sample dict] -> [sample dict]: the chain applied to a mini-batch, the `batch_apply` transform once for all samples."""
        cut = next(i for i, t in enumerate(self.transforms) if hasattr(t, "batch_apply"))
        samples = []
        for data in items:
            for t in self.transforms[:cut]:
                data = t(data)
            samples.append(data)
        samples = self.transforms[cut].batch_apply(samples)
        out = []
        for data in samples:
            for t in self.transforms[cut + 1:]:
                data = t(data)
            out.append(data)
        return out


# ---- the reference's own transforms ---------------------------------------------------------------------------------

class LoadGraphAndFilterByRandomRadiusd(MapTransform):
    """Graph CSV -> grey image per key, key i rendered at image_resolutions[i] with min_radius[i]; the first key creates the
    dropout `blackdict`, later keys reuse it (reference :358-387). Rendering is the HIP rasteriser (bit-exact with the
    reference's matplotlib/Agg output); tensors are returned on the GPU.

    Fast path (max_dropout_prob == 0, no blackdict file -- the segmentation configs): the CSV is parsed by the native
    reader (octa_csv_parse_edges, the reference's "Legacy" string branch of tree2img.py:73-76 with strtod) and the radius
    window is applied on the device; the global `random` stream is advanced exactly as the reference's loop would (one
    draw for the dropout probability on the first key, one draw per in-range edge on every key).
    """

    def __init__(self, keys, allow_missing_keys: bool = False, image_resolutions=[[304, 304]], min_radius=[0], max_dropout_prob=0,
                 MIP_axis=2) -> None:
        super().__init__(keys, allow_missing_keys)
        self.min_radius = min_radius
        self.image_resolutions = image_resolutions
        self.max_dropout_prob = max_dropout_prob
        self.MIP_axis = MIP_axis

    def rng_streams(self, has_background=True):
        return {"python"}           # tree2img.py:62,78: the dropout draws come from the global `random`

    def __call__(self, data):
        data = dict(data)
        if "blackdict" in data:
            with open(data["blackdict"], mode="rb") as file:
                blackdict = pickle.load(file)
        else:
            blackdict = None
        fast = self.max_dropout_prob == 0 and blackdict is None and torch.cuda.is_available()
        for i, key in enumerate(self.keys):
            if key not in data:
                if self.allow_missing_keys:
                    continue
                raise KeyError(f"LoadGraphAndFilterByRandomRadiusd: key {key!r} is missing")
            path = data[key]
            if fast:
                e, d_edges = load_graph_cached(path)
                lo = float(self.min_radius[i])
                n_in = int(np.count_nonzero((e[:, 6] >= lo) & (e[:, 6] <= 1.0)))
                # p = random() ** 10 * max_dropout_prob on the first key (tree2img.py:62), then `random() < p` per surviving edge (:78)
                advance_python_random(n_in + (1 if i == 0 else 0))
                img = tree2img.rasterize_edges_device(d_edges, np.array([0, len(e)]), self.image_resolutions[i], self.MIP_axis,
                                                      min_radius=lo, max_radius=1.0)[0]
                data[key] = img.to(torch.float32)
            else:
                with open(path, newline='') as csvfile:
                    f = list(csv.DictReader(csvfile))
                img, blackdict = rasterize_forest(f, self.image_resolutions[i], self.MIP_axis, min_radius=self.min_radius[i],
                                                  max_dropout_prob=self.max_dropout_prob, blackdict=blackdict)
                data[key] = torch.tensor(img.astype(np.float32)).to(default_device())
        return data


class ToGrayScaled(MapTransform):
    """RGB -> grey with Pillow's "L" weights, (19595 R + 38470 G + 7471 B + 0x8000) >> 16 on uint8-truncated values
    (reference :389-400 goes through PIL.Image.convert("L")); single-channel inputs pass through truncated to uint8."""

    def __call__(self, data):
        data = dict(data)
        for key in self.present(data):
            x = data[key]
            u = x.to(torch.uint8).to(torch.int64)         # astype(np.uint8): truncation, wraps like numpy for out-of-range values
            if x.dim() == 3 and x.shape[-1] in (3, 4):
                u = (19595 * u[..., 0] + 38470 * u[..., 1] + 7471 * u[..., 2] + 0x8000) >> 16
            data[key] = u.to(torch.float32)
        return data


class SpeckleBrightnesd(MapTransform):
    """Speckle component of the noise model (reference :25-42): a 9x9 control grid in [0.5, 1) bilinearly upsampled to the
    image, R = C - U (1 - C), img * R, then divided by the max and shifted by the min. The two random tensors come from
    torch's CPU generator exactly as in the reference (same values for the same torch.manual_seed), the arithmetic runs
    on the tensor's device."""

    def rng_streams(self, has_background=True):
        return {"torch"}

    def __call__(self, data):
        data = dict(data)
        for key in self.present(data):
            img = data[key]
            c = torch.rand((1, 1, 9, 9)) * 0.5 + 0.5
            if img.is_cuda and img.dim() == 3 and img.shape[0] == 1:
                from .gpu_augment import speckle_brightness             # csrc/augment.hip: two streaming passes, same draws
                u = torch.rand((1,) + tuple(img.shape[-2:]))
                data[key] = speckle_brightness(img.float(), c.reshape(1, 9, 9).to(img.device), u.to(img.device)).to(img.dtype)
                continue
            C = torch.nn.functional.interpolate(c, size=img.shape[-2:], mode="bilinear").squeeze(0)
            R = C - (torch.rand_like(C) * (1 - C))
            img = img * R.to(img.device)
            img = img / img.max()
            img = img - img.min()
            data[key] = img
        return data


class AddRandomBackgroundNoised(MapTransform):
    """img = max(img, background * U(0,1)) with uniform noise standing in for a missing background tile (reference
    :498-516); the per-pixel factors come from numpy's global stream, as in the reference."""

    def __init__(self, keys, delete_background=True) -> None:
        super().__init__(keys, True)
        self.delete_background = delete_background

    def rng_streams(self, has_background=True):
        return {"numpy"} if has_background else {"numpy", "torch"}      # torch.rand stands in for a missing background tile

    def __call__(self, data):
        data = dict(data)
        for key in self.keys:
            if key in data:
                img = data[key]
                # (torch.rand stands in for a missing tile: this transform then shares torch's stream with SpeckleBrightnesd and
                # must not be reordered against it -- image_dataset.ListDataset.get_batch checks for the key)
                noise = data["background"].to(img.device) if "background" in data else torch.rand(img.shape).to(img.device)
                speckle = torch.from_numpy(np.random.uniform(0, 1, tuple(img.shape))).to(img.device)
                if img.is_cuda and img.dtype == torch.float32 and noise.dtype == torch.float32 and noise.shape == img.shape:
                    from .gpu_augment import background_noise           # csrc/augment.hip
                    data[key] = background_noise(img, noise, speckle)
                else:
                    data[key] = torch.maximum(img, noise * speckle)      # float64 product, as torch promotes in the reference
        if self.delete_background and "background" in data:
            del data["background"]
        return data


# ---- the augmentation of Menten et al. (MICCAI 2022): the reference's comparison baseline (:44-325) -----------------------------------
# Draws and host restatement: data/menten.py; kernels: csrc/menten.hip through data/gpu_augment.py. CUDA tensors of the layouts the loader
# produces (image [1, H, W]; for the motion step a label of exactly [1, 4H, 4W]) go through the kernels. CPU tensors and other layouts take
# the host restatement (numpy + scipy.ndimage, bit-identical to the reference); a CUDA tensor that has to take it says so.

class HostFallbackError(RuntimeError):
    pass


_HOST_FALLBACK_WARNED = set()


def _host_fallback(where, why, kernels="csrc/menten.hip", host="numpy / scipy"):
    """A CUDA tensor is about to be copied to the host and back because its layout is outside the HIP kernels: warn ONCE per (place,
    reason), raise under OCTA_STRICT=1 (the convention of models/networks.py `_vendor_fallback`). `kernels` / `host` name the source file
    the sample leaves and what the host restatement runs on."""
    import os
    import warnings
    msg = (f"{where}: this CUDA sample leaves the HIP kernels ({kernels}) for the host restatement ({host}, a copy down and up): "
           f"{why}. Results stay correct, speed does not; OCTA_STRICT=1 turns this into an error.")
    if os.environ.get("OCTA_STRICT", "0") == "1":
        raise HostFallbackError(msg)
    if (where, why) not in _HOST_FALLBACK_WARNED:
        _HOST_FALLBACK_WARNED.add((where, why))
        warnings.warn(msg, RuntimeWarning, stacklevel=3)


def _device_image(x):
    """None when `x` is a CUDA image [1, H, W] in float32 / float64 (the kernels' layout), else the reason it is not."""
    if x.dim() != 3 or x.shape[0] != 1:
        return f"shape {tuple(x.shape)} is not [1, H, W]"
    if x.dtype not in (torch.float32, torch.float64):
        return f"dtype {x.dtype} is neither float32 nor float64"
    return None


def _through_host(x, fn):
    """The reference's `img.squeeze().numpy()` -> fn -> `torch.tensor(img).view(img_shape)`, on a copy, back on x's device."""
    out = fn(x.detach().cpu().squeeze().numpy().copy())
    return torch.tensor(out).view(x.shape).to(x.device)


class BinomialVesselNoised(MapTransform):
    """Binomial + quantum noise of Menten et al. (reference :44-102): a Bernoulli(0.1) field dilated once by the 3x3 cross, attenuated by 0.7
    per ring sqrt((i - H/2)^2 + (j - W/2)^2) < r - 3m (m = 0..4), blurred (scipy gaussian_filter, `reflect`), scaled, added with
    uniform(0, 0.2) noise, divided by 1 + scaling / 1.5 and clipped. Output float64 in the input's shape."""

    def __init__(self, keys, allow_missing_keys: bool = False, vessel_noise_scaling=0.5, vessel_noise_blur=1.0, r=48) -> None:
        super().__init__(keys, allow_missing_keys)
        self.vessel_noise_scaling = vessel_noise_scaling
        self.vessel_noise_blur = vessel_noise_blur
        self.r = r

    def rng_streams(self, has_background=True):
        return {"numpy"}

    def __call__(self, data):
        from . import menten
        data = dict(data)
        for key in self.keys:
            if key in data or not self.allow_missing_keys:
                img = data[key]
                why = None
                if img.is_cuda:
                    why = _device_image(img)
                    if why is None and not (0 < float(self.vessel_noise_blur) and menten.gaussian_radius(self.vessel_noise_blur) <= 512):
                        why = f"vessel_noise_blur {self.vessel_noise_blur} is outside the kernel's radius range"
                    if why is not None:
                        _host_fallback("BinomialVesselNoised", why)
                if img.is_cuda and why is None:
                    from .gpu_augment import menten_vessel_noise
                    bern, quantum = menten.vessel_noise_draws(tuple(img.shape[-2:]))
                    dev = img.device
                    data[key] = menten_vessel_noise(img, torch.from_numpy(bern).to(dev).unsqueeze(0), torch.from_numpy(quantum).to(dev).unsqueeze(0),
                                                    self.vessel_noise_blur, self.vessel_noise_scaling, self.r)
                else:
                    data[key] = _through_host(img, lambda a: menten.vessel_noise_host(a, self.vessel_noise_scaling, self.vessel_noise_blur, self.r))
        return data


class AddVitreousFloater(MapTransform):
    """Vitreous floater of Menten et al. (reference :104-185): with probability floater_chance a random walk of Bresenham segments, dilated
    `dilations` times by the 3x3 cross and blurred with sigma 10, darkens the image: img * (1 - floater), float64. Without a floater the image
    comes back unchanged in its own dtype. As in the reference, the drawn opacity has no effect (the dilation makes the mask boolean) and
    the mask is allocated as (W, H), so a floater on a non-square image raises numpy's broadcasting ValueError -- after its draws."""

    def __init__(self, keys, allow_missing_keys: bool = False, floater_chance: float = 0.1, floater_opacity_interval=(0.5, 1.0),
                 floater_segments_interval=(10, 20), dilations_interval=(10, 30)) -> None:
        super().__init__(keys, allow_missing_keys)
        self.floater_chance = floater_chance
        self.floater_opacity_interval = floater_opacity_interval
        self.floater_segments_interval = floater_segments_interval
        self.dilations_interval = dilations_interval

    def rng_streams(self, has_background=True):
        return {"numpy"}

    def __call__(self, data):
        from . import menten
        data = dict(data)
        for key in self.keys:
            if key in data or not self.allow_missing_keys:
                img = data[key]
                if img.squeeze().dim() != 2:
                    raise ValueError(f"AddVitreousFloater: {tuple(img.shape)} does not squeeze to a 2-D image")
                H, W = img.squeeze().shape
                draws = menten.floater_draws(H, W, self.floater_chance, self.floater_opacity_interval, self.floater_segments_interval,
                                             self.dilations_interval)
                if draws is None:
                    data[key] = img.clone()
                    continue
                points, opacity, dilations = draws
                why = None
                if img.is_cuda:
                    why = _device_image(img)
                    if why is None and H != W:
                        # the reference's `img * (1 - floater)` with floater of shape (W, H)
                        raise ValueError(f"operands could not be broadcast together with shapes ({H},{W}) ({W},{H}) ")
                    if why is None and (dilations < 1 or W > 4096):
                        why = f"dilations {dilations} / size {W} outside the kernel's range"
                    if why is not None:
                        _host_fallback("AddVitreousFloater", why)
                if img.is_cuda and why is None:
                    from .gpu_augment import menten_floater
                    segs = points if opacity != 0 else points[:1]           # an opacity of exactly 0 leaves the mask empty
                    data[key] = menten_floater(img.double(), [segs], [dilations])
                else:
                    data[key] = _through_host(img, lambda a: menten.floater_host(a, draws))
        return data


class AddMotionArtifact(MapTransform):
    """Motion artifacts of Menten et al. (reference :187-302): up to no_h_cuts - 1 horizontal cuts, each a shear (rows below shifted right,
    zero filled), stretch (one row repeated), buckle (rows repeated from above) or whiteout (rows of uniform(0.5, 1) noise, image only) at a
    random row; the label (four times the image's resolution) gets the same cut at 4 x position and 4 x amount. dtypes are kept; new tensors
    are returned (the reference writes through `.numpy()` into its inputs). As in the reference, `__call__` does not hand `no_h_cuts` on to
    `add_motion_artifact`, whose own default (3) therefore always applies."""

    def __init__(self, img_key, gt_key, artifacts={'shear': 0.3, 'stretch': 0.3, 'buckle': 0.3, 'whiteout': 0.1}, grace_margin: int = 10,
                 max_shear: int = 5, max_stretch: int = 5, max_buckle: int = 5, max_whiteout: int = 1, no_h_cuts: int = 3) -> None:
        super().__init__([img_key, gt_key], False)
        self.img_key = img_key
        self.gt_key = gt_key
        self.artifacts = artifacts
        self.grace_margin = grace_margin
        self.max_shear = max_shear
        self.max_stretch = max_stretch
        self.max_buckle = max_buckle
        self.max_whiteout = max_whiteout
        self.no_h_cuts = no_h_cuts

    def rng_streams(self, has_background=True):
        return {"numpy"}

    def __call__(self, data):
        from . import menten
        data = dict(data)
        img, gt = data[self.img_key], data[self.gt_key]
        why = None
        if img.is_cuda or gt.is_cuda:
            ok = lambda t: t.is_cuda and t.dim() == 3 and t.shape[0] == 1 and t.is_floating_point() and t.element_size() in (4, 8)
            if not (ok(img) and ok(gt)):
                why = f"image {tuple(img.shape)} {img.dtype} on {img.device} / label {tuple(gt.shape)} {gt.dtype} on {gt.device} are not [1, H, W] CUDA tensors of 4- or 8-byte floats"
            elif (gt.shape[1], gt.shape[2]) != (4 * img.shape[1], 4 * img.shape[2]):
                why = f"label {tuple(gt.shape)} is not [1, 4H, 4W] of image {tuple(img.shape)}"
            if why is not None:
                _host_fallback("AddMotionArtifact", why)
        h, w = img.squeeze().shape
        cuts = menten.motion_draws(h, w, self.artifacts, self.grace_margin, self.max_shear, self.max_stretch, self.max_buckle, self.max_whiteout)
        if img.is_cuda and gt.is_cuda and why is None:
            from .gpu_augment import menten_motion
            H, W = img.shape[1:]
            table, white = menten.fold_cuts(H, W, cuts, 1)
            data[self.img_key] = menten_motion(img, table, white)
            data[self.gt_key] = menten_motion(gt, menten.fold_cuts(H, W, cuts, 4)[0])
        else:
            a, g = menten.motion_host(img.detach().cpu().squeeze().numpy().copy(), gt.detach().cpu().squeeze().numpy().copy(), cuts)
            data[self.img_key] = torch.tensor(a).view(img.shape).to(img.device)
            data[self.gt_key] = torch.tensor(g).view(gt.shape).to(gt.device)
        return data


class MentenAugmentationd(MapTransform):
    """BinomialVesselNoised -> AddVitreousFloater -> AddMotionArtifact with their defaults (reference :304-325), the augmentation of

    Physiology-Based Simulation of the Retinal Vasculature Enables Annotation-Free Segmentation of OCT Angiographs
    M. J. Menten, J. C. Paetzold, A. Dima, B. H. Menze, B. Knier, D. Rueckert, MICCAI 2022

    which the reference's paper compares its noise model against (configs/config_ves_seg-S_Menten_aug.yml)."""

    def __init__(self, img_key: str, gt_key: str) -> None:
        super().__init__(keys=[img_key, gt_key], allow_missing_keys=False)
        self.img_key = img_key
        self.gt_key = gt_key
        self.binomialVesselNoised = BinomialVesselNoised([img_key], allow_missing_keys=True)
        self.vitreousFloater = AddVitreousFloater([img_key], allow_missing_keys=True)
        self.add_motion_artifact = AddMotionArtifact(img_key, gt_key)

    def rng_streams(self, has_background=True):
        return {"numpy"}

    def __call__(self, data):
        data = self.binomialVesselNoised(data)
        data = self.vitreousFloater(data)
        data = self.add_motion_artifact(data)
        return data


# ---- the reference's noise model: the "random augmentation" configuration (configs/config_ves_seg-S_RA.yml; reference :435-496) -------------
# Draws and host restatement: data/noise_model.py; kernel: csrc/noise_model.hip through data/gpu_augment.py.

class NoiseModeld(MapTransform):
    """The paper's handcrafted noise model (reference :435-475 -> models/noise_model.py NoiseModel.forward, adversarial=False): background
    vessels `max(I, I_d lambda_delta Delta)`, speckle `(lambda_speckle N + 1 - lambda_speckle)`, contrast `pow(. + 1e-6, Gamma)`, where Delta and
    N are per-pixel Beta variates whose two shape maps, like Gamma, are bicubic upsamplings of random gh x gw control grids. The sample must
    hold a `background` tensor of the image's shape; it stays in the sample. One `random.random() < prob` is drawn per call, at prob 1 too.
    As in the reference, a key that is missing raises whatever allow_missing_keys says; `alpha` is the step size of the adversarial mode,
    which is not part of this package, and is only kept.

    CPU tensors take the host restatement (data/noise_model.py), bit-identical to the reference's class for the same torch.manual_seed.
    CUDA float32 tensors [1, H, W] with downsample_factor 1 take csrc/noise_model.hip: the control grids are drawn on the host from torch's
    global generator exactly as on the host path (the FIRST call of an instance draws them twice, as the reference does), then ONE 64-bit
    seed is drawn from the same generator and the per-pixel Beta fields are made on the device by a counter-based generator keyed with it.
    torch.manual_seed therefore fixes a run on either path, and both paths use the same control points -- but they leave torch's generator
    at DIFFERENT positions: the host path consumes two H x W Beta fields from it per call, the device path one integer. Whatever draws from
    torch's generator afterwards differs between a host and a device run; the per-pixel fields differ too (same distribution, other bits).
    Any other CUDA layout takes the host restatement and says so (warning once; error under OCTA_STRICT=1)."""

    def __init__(self, keys, prob=1, allow_missing_keys: bool = False, grid_size=(9, 9), lambda_delta=1, lambda_speckle=0.7, lambda_gamma=0.3,
                 alpha=0.2, downsample_factor=1) -> None:
        super().__init__(keys, allow_missing_keys)
        from .noise_model import NoiseModelDraws
        self.prob = prob
        self.grid_size = tuple(grid_size)
        self.lambda_delta, self.lambda_speckle, self.lambda_gamma = lambda_delta, lambda_speckle, lambda_gamma
        self.alpha = alpha
        self.downsample_factor = downsample_factor
        self.draws = NoiseModelDraws(self.grid_size)

    def rng_streams(self, has_background=True):
        return {"python", "torch"}

    def _why_not_device(self, img, background):
        if img.dim() != 3 or img.shape[0] != 1:
            return f"shape {tuple(img.shape)} is not [1, H, W]"
        if self.downsample_factor != 1:
            return f"downsample_factor {self.downsample_factor} is not 1"
        if img.dtype != torch.float32 or background.dtype != torch.float32:
            return f"dtypes {img.dtype} / {background.dtype} (background) are not float32"
        if not background.is_cuda or background.shape != img.shape:
            return f"background {tuple(background.shape)} on {background.device} does not match the image {tuple(img.shape)} on {img.device}"
        return None

    def __call__(self, data):
        from . import noise_model as nm
        data = dict(data)
        if _py_random.random() < self.prob:
            for key in self.keys:
                img, background = data[key], data["background"]
                why = None
                if img.is_cuda:
                    why = self._why_not_device(img, background)
                    if why is not None:
                        _host_fallback("NoiseModeld", why, kernels="csrc/noise_model.hip", host="torch on the CPU")
                if img.is_cuda and why is None:
                    from .gpu_augment import noise_model
                    grids = torch.cat(self.draws.control_points(1, img.dtype), dim=1)           # [1, 5, gh, gw]
                    seed = int(torch.empty((), dtype=torch.int64).random_().item())
                    data[key] = noise_model(img, background, grids, seed, self.lambda_delta, self.lambda_speckle, self.lambda_gamma)
                else:
                    I, I_d = img.detach().cpu().unsqueeze(0), background.detach().cpu().unsqueeze(0)  # noqa: E741
                    out = nm.noise_model_host(I, I_d, self.draws.control_points(1, I.dtype), self.lambda_delta, self.lambda_speckle,
                                              self.lambda_gamma, self.downsample_factor)
                    data[key] = out.squeeze(0).detach().to(img.device)
        return data


class RandomDecreaseResolutiond(MapTransform):
    """Lower the resolution by a random factor and bring the image back to its size, both by nearest-neighbour resampling (reference :477-496):
    `random.uniform(0, 1) < p`, then per key `factor = random.uniform(max_factor, 1)`, interpolate(scale_factor=factor), interpolate(size).
    As in the reference, allow_missing_keys is set but a missing key raises. CPU tensors go through torch's two interpolations; on CUDA
    tensors the two resamples are one gather per axis with index tables that torch's CPU nearest kernel itself produced
    (data/noise_model.py nearest_roundtrip_tables), so the result is the CPU result exactly, not the device kernel's own rounding."""

    def __init__(self, keys, p=1, max_factor=0.25) -> None:
        super().__init__(keys, True)
        self.max_factor = max_factor
        self.p = p

    def rng_streams(self, has_background=True):
        return {"python"}

    def __call__(self, data):
        from .noise_model import nearest_roundtrip_tables
        data = dict(data)
        if _py_random.uniform(0, 1) < self.p:
            for key in self.keys:
                d = data[key]
                factor = _py_random.uniform(self.max_factor, 1)
                if d.is_cuda:
                    for axis, table in enumerate(nearest_roundtrip_tables(d.shape[1:], factor)):
                        d = d.index_select(axis + 1, table.to(d.device))
                else:
                    d = torch.nn.functional.interpolate(d.unsqueeze(0), scale_factor=factor)
                    d = torch.nn.functional.interpolate(d, size=data[key].shape[1:]).squeeze(0)
                data[key] = d
        return data


class RandCropOrPadd(MapTransform):
    """Random crop or zero pad by a random zoom factor (reference :543-585; the Giarratano set-up crops 1216 -> 360 with both factors 0.2965),
    restated literally. Every call draws `random.uniform(0, 1)` once from the global `random`; nothing else happens unless it is `< prob`.
    Then `factor = random.uniform(min_factor, max_factor)`:
      factor < 1: at the FIRST key only, s_x = int(shape[1] * factor), s_y = int(shape[2] * factor), then randint(0, shape[1] - s_x), then
        randint(0, shape[2] - s_y) (rows first); every later key takes the same two slices whatever its own shape: d[:, slice_x, slice_y];
      factor > 1, per key and without draws: a float32 zero frame [C, int(H * factor), int(W * factor)] on the tensor's device with the input
        copied in at (frame - size) // 2 per axis -- float32 whatever the input's dtype (the reference's frame is torch.zeros on the CPU);
      factor == 1: unchanged.
    A missing key raises KeyError, as the reference's indexing does. Slices and copies only, on CPU and device tensors alike. `offsets` keeps the
    (start_x, start_y) of the last crop, None after any other call (read by the tests and the fused chain's comparison)."""

    def __init__(self, keys, prob=0.1, min_factor=1, max_factor=1) -> None:
        super().__init__(keys)
        self.prob = prob
        self.min_factor = min_factor
        self.max_factor = max_factor
        self.offsets = None

    def rng_streams(self, has_background=True):
        return {"python"}

    def __call__(self, data):
        self.offsets = None
        data = dict(data)
        if _py_random.uniform(0, 1) < self.prob:
            factor = _py_random.uniform(self.min_factor, self.max_factor)
            slice_x = slice_y = None
            for k in self.keys:
                d = data[k]
                if factor < 1:
                    if slice_x is None:
                        s_x = int(d.shape[1] * factor)
                        s_y = int(d.shape[2] * factor)
                        start_x = _py_random.randint(0, d.shape[1] - s_x)
                        start_y = _py_random.randint(0, d.shape[2] - s_y)
                        slice_x = slice(start_x, start_x + s_x)
                        slice_y = slice(start_y, start_y + s_y)
                        self.offsets = (start_x, start_y)
                    d = d[:, slice_x, slice_y]
                elif factor > 1:
                    frame = torch.zeros((d.shape[0], int(d.shape[1] * factor), int(d.shape[2] * factor)), dtype=torch.float32, device=d.device)
                    start_x = (frame.shape[1] - d.shape[1]) // 2
                    start_y = (frame.shape[2] - d.shape[2]) // 2
                    frame[:, start_x:start_x + d.shape[1], start_y:start_y + d.shape[2]] = d.clone()
                    d = frame
                data[k] = d
        return data


class ImageToImageTranslationd(MapTransform):
    """Frozen-generator contrast adaptation (reference :327-356) -- on the GPU (the reference runs resnetGenerator9 inside
    CPU loader workers: 6.1 s per image). `model` may be passed directly; otherwise resnetGenerator9 weights
    are loaded from `model_path` (checkpoint dict with key 'model')."""

    def __init__(self, model_path=None, keys=("image",), model_config: dict = None, allow_missing_keys: bool = False,
                 model=None, device=None, amp=None) -> None:
        super().__init__(keys, allow_missing_keys)
        from ..models.base_model_abc import load_checkpoint_file
        from ..models.networks import MODEL_DICT
        if model is None:
            if model_config is not None and model_config.get("name", "resnetGenerator9") != "resnetGenerator9":
                raise NotImplementedError("only resnetGenerator9 translation models are on the MI355X hot path")
            model = MODEL_DICT["resnetGenerator9"]()
            if model_path is not None:
                ckpt = load_checkpoint_file(model_path, "cpu")
                model.load_state_dict(ckpt["model"])
                import sys
                print(f"Loaded network weights from epoch {ckpt['epoch']}.", file=sys.stderr)
        self.device = torch.device(device) if device is not None else default_device()
        self.model = model.to(self.device).eval().requires_grad_(False)
        # bf16 autocast on the GPU: the generator's 3x3 stages run the MFMA convolution kernels and its stems the thin-conv
        # kernels (models/networks.py), as in the GAN-seg training step; `amp: false` keeps the fp32 torch modules
        self.amp = (self.device.type == "cuda") if amp is None else (bool(amp) and self.device.type == "cuda")

    def _translate(self, x):
        with torch.no_grad(), torch.autocast(device_type=self.device.type, dtype=torch.bfloat16, enabled=self.amp):
            return self.model(x.float().to(self.device)).float()

    def __call__(self, data):
        data = dict(data)
        for key in self.present(data):
            data[key] = self._translate(data[key].unsqueeze(0)).squeeze(0)
        return data

    def batch_apply(self, samples):
        """The same transform on a list of samples with ONE generator pass per key over the stacked mini-batch (InstanceNorm is
        per sample, so each image gets what its own pass would give)."""
        samples = [dict(d) for d in samples]
        for key in self.keys:
            have = [d for d in samples if key in d]
            if len(have) != len(samples) and not self.allow_missing_keys:
                raise KeyError(f"ImageToImageTranslationd: key {key!r} is missing from a sample")
            if not have:
                continue
            if len({tuple(d[key].shape) for d in have}) == 1:
                y = self._translate(torch.stack([d[key] for d in have]))
                for i, d in enumerate(have):
                    d[key] = y[i]
            else:
                for d in have:
                    d[key] = self._translate(d[key].unsqueeze(0)).squeeze(0)
        return samples


# ---- MONAI transforms named by the configs (restated; see the module docstring) ------------------------------------------------

class LoadImaged(MapTransform):
    """PNG -> float32 tensor on the GPU. MONAI's PILReader hands images over with the first two axes swapped (its
    `reverse_indexing`: [W, H(, C)]); the configs undo that with Rotate90d(k=1) + Flipd(spatial_axis=0), so the swap is kept.
    `.nii` / `.nii.gz` (octa_autosegmentation_amd/nifti.py) and `.npy` volumes arrive in their stored axis order: only the PIL reader
    swaps."""

    def __init__(self, keys, allow_missing_keys: bool = False, image_only: bool = True, **unused) -> None:
        super().__init__(keys, allow_missing_keys)

    def __call__(self, data):
        from PIL import Image
        data = dict(data)
        for key in self.present(data):
            path = str(data[key])
            if path.endswith((".nii", ".nii.gz")):
                from .. import nifti
                a = nifti.read(path)[0]
            elif path.endswith(".npy"):
                a = np.load(path)
            else:
                a = np.asarray(Image.open(data[key]))
                if a.dtype == bool:
                    a = a.astype(np.uint8)
                a = np.swapaxes(a, 0, 1)
            data[key] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(default_device())
        return data


class ScaleIntensityd(MapTransform):
    def __init__(self, keys, minv=0.0, maxv=1.0, allow_missing_keys: bool = False, **unused) -> None:
        super().__init__(keys, allow_missing_keys)
        self.minv, self.maxv = minv, maxv

    def __call__(self, data):
        data = dict(data)
        for key in self.present(data):
            x = data[key].to(torch.float32)
            mn, mx = x.min(), x.max()
            span = mx - mn
            scaled = (x - mn) / torch.where(span > 0, span, torch.ones_like(span)) * (self.maxv - self.minv) + self.minv
            data[key] = torch.where(span > 0, scaled, x * self.minv)      # constant image: MONAI returns arr * minv
        return data


class EnsureChannelFirstd(MapTransform):
    def __init__(self, keys, channel_dim=None, strict_check: bool = True, allow_missing_keys: bool = False, **unused) -> None:
        super().__init__(keys, allow_missing_keys)
        self.channel_dim = channel_dim

    def __call__(self, data):
        data = dict(data)
        for key in self.present(data):
            x = data[key]
            if self.channel_dim == "no_channel" or x.dim() == 2:
                x = x.unsqueeze(0)
            elif isinstance(self.channel_dim, int):
                x = x.movedim(self.channel_dim, 0)
            data[key] = x
        return data


class Resized(MapTransform):
    def __init__(self, keys, spatial_size, mode="area", allow_missing_keys: bool = False, align_corners=None, **unused) -> None:
        super().__init__(keys, allow_missing_keys)
        self.size, self.mode, self.align_corners = [int(v) for v in spatial_size], mode, align_corners

    def __call__(self, data):
        data = dict(data)
        for key in self.present(data):
            x = data[key]
            if list(x.shape[1:]) == self.size:
                continue
            data[key] = _interpolate(x, self.size, self.mode, self.align_corners)
        return data


def _interpolate(x, size, mode, align_corners):
    """Channel-first [C, *spatial] -> float32 [C, *size] by torch's interpolation (MONAI Resize without anti-aliasing)."""
    kw = {"align_corners": align_corners} if mode in ("bilinear", "bicubic") else {}
    return torch.nn.functional.interpolate(x.float().unsqueeze(0), size=size, mode=mode, **kw).squeeze(0)


class Resize:
    """MONAI's Resize of a post-processing chain (configs/config_oof.yml): channel-first [C, H, W] -> float32 [C, *spatial_size],
    `mode` area by default, no anti-aliasing; the interpolation of Resized."""

    def __init__(self, spatial_size, mode="area", align_corners=None, **unused):
        self.size, self.mode, self.align_corners = [int(v) for v in spatial_size], mode, align_corners

    def __call__(self, x):
        if list(x.shape[1:]) == self.size:
            return x.float()
        return _interpolate(x, self.size, self.mode, self.align_corners)


def _spatial_dims(axes):
    axes = [axes] if isinstance(axes, int) else list(axes)
    return [a + 1 for a in axes]                     # channel-first tensors: spatial axis a is tensor dim a + 1


class Flipd(MapTransform):
    def __init__(self, keys, spatial_axis=None, allow_missing_keys: bool = False, **unused) -> None:
        super().__init__(keys, allow_missing_keys)
        self.spatial_axis = spatial_axis

    def flip(self, x):
        dims = list(range(1, x.dim())) if self.spatial_axis is None else _spatial_dims(self.spatial_axis)
        return torch.flip(x, dims)

    def __call__(self, data):
        data = dict(data)
        for key in self.present(data):
            data[key] = self.flip(data[key])
        return data


class RandFlipd(Flipd, Randomizable):
    def __init__(self, keys, prob=0.1, spatial_axis=None, allow_missing_keys: bool = False, **unused) -> None:
        Flipd.__init__(self, keys, spatial_axis, allow_missing_keys)
        self.prob = prob

    def __call__(self, data):
        data = dict(data)
        do = self.R.rand() < self.prob
        for key in self.present(data):
            if do:
                data[key] = self.flip(data[key])
        return data


class Rotate90d(MapTransform):
    def __init__(self, keys, k=1, spatial_axes=(0, 1), allow_missing_keys: bool = False, **unused) -> None:
        super().__init__(keys, allow_missing_keys)
        self.k, self.spatial_axes = k, tuple(spatial_axes)

    def __call__(self, data):
        data = dict(data)
        for key in self.present(data):
            data[key] = torch.rot90(data[key], self.k, _spatial_dims(self.spatial_axes))
        return data


class RandRotate90d(MapTransform, Randomizable):
    def __init__(self, keys, prob=0.1, max_k=3, spatial_axes=(0, 1), allow_missing_keys: bool = False, **unused) -> None:
        MapTransform.__init__(self, keys, allow_missing_keys)
        self.prob, self.max_k, self.spatial_axes = prob, max_k, tuple(spatial_axes)

    def __call__(self, data):
        data = dict(data)
        k = self.R.randint(self.max_k) + 1
        do = self.R.rand() < self.prob
        for key in self.present(data):
            if do:
                data[key] = torch.rot90(data[key], k, _spatial_dims(self.spatial_axes))
        return data


def rotate2d(x, angle, mode="bilinear", padding_mode="zeros", align_corners=False):
    """Rotation of a channel-first 2-D image about its centre, output size = input size (MONAI Rotate with keep_size)."""
    c, s = float(np.cos(angle)), float(np.sin(angle))
    H, W = x.shape[-2:]
    # normalised coordinates are anisotropic on non-square images: a rotation in pixel space is [[c, -s W/H... ]] there
    theta = torch.tensor([[[c, -s * H / W, 0.0], [s * W / H, c, 0.0]]], dtype=torch.float32, device=x.device)
    grid = torch.nn.functional.affine_grid(theta, (1, x.shape[0], H, W), align_corners=align_corners)
    return torch.nn.functional.grid_sample(x.float().unsqueeze(0), grid, mode=mode, padding_mode=padding_mode, align_corners=align_corners).squeeze(0)


class RandRotated(MapTransform, Randomizable):
    def __init__(self, keys, range_x=0.0, range_y=0.0, range_z=0.0, prob=0.1, keep_size=True, mode="bilinear", padding_mode="border",
                 align_corners=False, allow_missing_keys: bool = False, **unused) -> None:
        MapTransform.__init__(self, keys, allow_missing_keys)
        rng = lambda r: (-abs(r), abs(r)) if np.isscalar(r) else tuple(sorted(r))
        self.range_x, self.range_y, self.range_z = rng(range_x), rng(range_y), rng(range_z)
        self.prob, self.mode, self.padding_mode, self.align_corners = prob, mode, padding_mode, align_corners
        if not keep_size:
            raise NotImplementedError("RandRotated(keep_size=False) is not used by the OCTA configs")

    def __call__(self, data):
        data = dict(data)
        do = self.R.rand() < self.prob
        if do:
            x = self.R.uniform(low=self.range_x[0], high=self.range_x[1])
            self.R.uniform(low=self.range_y[0], high=self.range_y[1])
            self.R.uniform(low=self.range_z[0], high=self.range_z[1])
        for key in self.present(data):
            if do:
                data[key] = rotate2d(data[key], x, self.mode, self.padding_mode, self.align_corners)
        return data


class AsDiscreted(MapTransform):
    def __init__(self, keys, threshold=None, argmax=False, allow_missing_keys: bool = False, **unused) -> None:
        super().__init__(keys, allow_missing_keys)
        self.threshold, self.argmax = threshold, argmax

    def __call__(self, data):
        data = dict(data)
        for key in self.present(data):
            x = data[key]
            if self.argmax:
                x = x.argmax(dim=0, keepdim=True).to(torch.float32)
            if self.threshold is not None:
                x = (x >= self.threshold).to(x.dtype if x.is_floating_point() else torch.float32)
            data[key] = x
        return data


class CastToTyped(MapTransform):
    def __init__(self, keys, dtype=torch.float32, allow_missing_keys: bool = False) -> None:
        super().__init__(keys, allow_missing_keys)
        self.dtype = dtype

    def __call__(self, data):
        data = dict(data)
        dts = self.dtype if isinstance(self.dtype, (list, tuple)) else [self.dtype] * len(self.keys)
        for key, dt in zip(self.keys, dts):
            if key in data:
                data[key] = data[key].to(dt)
            elif not self.allow_missing_keys:
                raise KeyError(f"CastToTyped: key {key!r} is missing")
        return data


class SelectSlice(MapTransform):
    """`data[key][slices]` with one slice per `[start, end]` pair of slice_selection, applied from dim 0 (the 3-D reconstruction set-up
    keeps depth slices 5 .. -4 of the channel-first label volume). None = identity (the reference raises AttributeError there)."""

    def __init__(self, keys, allow_missing_keys: bool = False, slice_selection=None) -> None:
        super().__init__(keys, allow_missing_keys)
        self.slice_selection = tuple(slice(s, e) for s, e in slice_selection) if slice_selection else None

    def __call__(self, data):
        if self.slice_selection is None:
            return data
        data = dict(data)
        for key in self.present(data):
            data[key] = data[key][self.slice_selection]
        return data


# ---- post-processing (array transforms applied to one decollated sample, configs `post_processing`) ------------------

class Activations:
    def __init__(self, sigmoid=False, softmax=False, **unused):
        self.sigmoid, self.softmax = sigmoid, softmax

    def __call__(self, x):
        if self.sigmoid:
            x = torch.sigmoid(x.float())
        if self.softmax:
            x = torch.softmax(x.float(), dim=0)
        return x


class AsDiscrete:
    def __init__(self, threshold=None, argmax=False, **unused):
        self.threshold, self.argmax = threshold, argmax

    def __call__(self, x):
        if self.argmax:
            x = x.argmax(dim=0, keepdim=True).to(torch.float32)
        if self.threshold is not None:
            x = (x >= self.threshold).to(torch.float32)
        return x


class RemoveSmallObjects:
    """Connected components smaller than min_size removed (MONAI -> skimage.morphology.remove_small_objects; connectivity 1
    = 4-neighbourhood). On the GPU through the union-find kernel of csrc/postproc.hip, bit-exact with scipy.ndimage.label +
    bincount (tests/test_postproc_gpu.py). independent_channels=False (MONAI's keyword): the leading axis of a [C,H,W] input is
    depth and the components are those of the volume (csrc/cc3d.hip; connectivity 1 / 2 / 3 = 6- / 18- / 26-neighbourhood)."""

    def __init__(self, min_size=64, connectivity=1, independent_channels=True, **unused):
        self.min_size, self.connectivity, self.independent_channels = int(min_size), int(connectivity), bool(independent_channels)

    def __call__(self, x):
        from ..models.postprocess import remove_small_objects_device
        if not x.is_cuda:
            raise RuntimeError("RemoveSmallObjects runs on the GPU (no CPU fallback)")
        keep = remove_small_objects_device((x != 0).to(torch.uint8), self.min_size, self.connectivity, independent_channels=self.independent_channels)
        return x * keep.to(x.dtype)


class KeepLargestConnectedComponent:
    """MONAI's KeepLargestConnectedComponent for ONE foreground label: input [1, *spatial] with 2 or 3 spatial dims, non-zero =
    foreground; everything outside the component with the most voxels is zeroed, dtype kept. A tie goes to the component whose first
    voxel comes first in C order (argmax(bincount(labels)[1:]) + 1 on skimage's raster-ordered labels). connectivity None = full.
    MONAI treats several non-zero values of a one-channel image as separate labels and keeps the largest component of each; this
    class does not: every non-zero value is the same foreground. applied_labels, is_onehot=True, independent=False,
    num_components != 1 and more than one channel raise NotImplementedError. GPU only (csrc/cc3d.hip)."""

    def __init__(self, applied_labels=None, is_onehot=None, independent=True, connectivity=None, num_components=1):
        for arg, bad in (("applied_labels", applied_labels is not None), ("is_onehot", bool(is_onehot)), ("independent", not independent),
                         ("num_components", num_components != 1)):
            if bad:
                raise NotImplementedError(f"KeepLargestConnectedComponent: {arg} is supported only at its default (one foreground label, one component)")
        self.connectivity = None if connectivity is None else int(connectivity)

    def __call__(self, x):
        from ..models.postprocess import keep_largest_component_device
        if not x.is_cuda:
            raise RuntimeError("KeepLargestConnectedComponent runs on the GPU (no CPU fallback)")
        if x.dim() not in (3, 4):
            raise NotImplementedError(f"KeepLargestConnectedComponent: the input must be [1, *spatial] with 2 or 3 spatial dims, got {tuple(x.shape)}")
        if x.shape[0] != 1:
            raise NotImplementedError(f"KeepLargestConnectedComponent: is_onehot / several channels ({x.shape[0]}) are not supported")
        keep = keep_largest_component_device(x[0], self.connectivity)
        return x * keep[None].to(x.dtype)


class RemoveOuterNoise:
    """The reference's RemoveOuterNoise (data/data_transforms.py:418-432): everything of a volume that is not 26-connected to its
    central plane goes. Literally: a boolean copy, plane `volume.shape[z_axis] // 2` OF DIM 0 filled (the reference indexes dim 0
    whatever z_axis is -- kept, so z_axis only picks the length that is halved, and an index past dim 0 raises IndexError as there),
    the largest 26-connected component of that (KeepLargestConnectedComponent), logical_and with the input. Returns torch.bool.
    GPU only (csrc/cc3d.hip)."""

    def __init__(self, z_axis=0, **unused):
        self.z_axis = int(z_axis)

    def __call__(self, volume):
        from ..models.postprocess import remove_outer_noise_device
        if not volume.is_cuda:
            raise RuntimeError("RemoveOuterNoise runs on the GPU (no CPU fallback)")
        return remove_outer_noise_device(volume, self.z_axis)


class CastToType:
    def __init__(self, dtype=torch.float32):
        self.dtype = dtype

    def __call__(self, x):
        return x.to(self.dtype)


class AsChannelLast:
    """[C, ...] -> [..., C] (MONAI's AsChannelLast): the depth slices of a 3-D prediction become the last axis of the volume."""

    def __init__(self, channel_dim=0, **unused):
        self.channel_dim = int(channel_dim)

    def __call__(self, x):
        return x.movedim(self.channel_dim, -1)


TRANSFORMS = {c.__name__: c for c in (
    LoadGraphAndFilterByRandomRadiusd, ToGrayScaled, SpeckleBrightnesd, AddRandomBackgroundNoised, ImageToImageTranslationd,
    BinomialVesselNoised, AddVitreousFloater, AddMotionArtifact, MentenAugmentationd, NoiseModeld, RandomDecreaseResolutiond, RandCropOrPadd,
    LoadImaged, ScaleIntensityd, EnsureChannelFirstd, Resized, Flipd, RandFlipd, Rotate90d, RandRotate90d, RandRotated, AsDiscreted,
    CastToTyped, SelectSlice, Activations, AsDiscrete, RemoveSmallObjects, KeepLargestConnectedComponent, RemoveOuterNoise, Resize, CastToType,
    AsChannelLast)}


def get_data_augmentations(aug_config, seed=None, dtype=torch.float32):
    """YAML list -> transform objects (reference data_transforms.py:587-611): `name` picks the class, the other entries
    are its keyword arguments; `dtype: dtype` placeholders of CastToType* become `dtype` (bf16 under AMP training -- the
    reference's fp16, image_dataset.py:46, is its CUDA autocast type); random transforms are seeded with `seed`.
    Names outside the hot path raise."""
    if aug_config is None:
        return []
    augs = []
    for aug_d in aug_config:
        aug_d = dict(aug_d)
        name = aug_d.pop("name")
        if name not in TRANSFORMS:
            raise NotImplementedError(f"transform {name} is outside the MI355X hot path (MONAI is not a dependency)")
        if name.startswith("CastToType"):
            islist = isinstance(aug_d["dtype"], list)
            types = [dtype if t == "dtype" else (getattr(torch, t) if isinstance(t, str) else t) for t in (aug_d["dtype"] if islist else [aug_d["dtype"]])]
            aug_d["dtype"] = types if islist else types[0]
        obj = TRANSFORMS[name](**aug_d)
        if isinstance(obj, Randomizable):
            obj.set_random_state(seed=seed)
        augs.append(obj)
    return augs
