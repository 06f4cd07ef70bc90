"""tools/make_golden_skrgan.py -- generates tests/golden/skrgan_golden.npz: the reference's models/skrgan.py (sigma 2, the
hard-coded thresholds 64 / 64, connectivity 1) on a stand-in for the absent scikit-image -- tools/skr_scipy.py, registered as
`skimage.morphology`. Parity with scikit-image itself is not pinned.

Runs ONLY in the build container: imports /root/reference/models/skrgan.py at run time (nothing of it is committed). The five
inputs of the OOF fixtures (tests/test_oof.py CASES: odd 91 x 97, even 64 x 48, octa 304^2, crop 400^2, full 1216^2) are reused,
not stored again; tiny uint8 inputs are added (img = u8.astype(float32) / float32(255)): r8x8 (exactly 64 pixels: the opening
leaves a constant, so `open` and `out` are NaN everywhere), r9x8 and r12x11 (72 and 132 pixels: the closing leaves a constant, `out`
is NaN), r20x23 (random), and steps
(20 x 26, six grey levels in 3 x 3 blocks: plateaus and ties).
Per case the four planes of the call -- `mag` the normalised Sobel magnitude (what gaussian_filter receives), `filt` the filtered
plane (what area_opening receives), `open` the normalised opened plane (what area_closing receives), `out` the output --, float32,
as `<case>_<plane>`: every `<case>_step`-th pixel of both axes (`out` of octa and even in full, for the end-to-end test), and
`<case>_sha`: SHA-256 of each FULL plane's bytes after `+ 0.0` and with every NaN made the same NaN, in that order. `w_sigma2` is
scipy's own `_gaussian_kernel1d(2, 0, 8)`.

Asserted here: the reference returns NaN everywhere for a constant input; octa and even keep at least one object behind the
configuration's post-processing (threshold 0.5, RemoveSmallObjects). Re-running rewrites the file byte for byte."""
import hashlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch
from scipy import ndimage as ndi
from scipy.ndimage._filters import _gaussian_kernel1d

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF = "/root/reference"
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import skr_scipy  # noqa: E402
from make_golden_frangi import write_npz  # noqa: E402

TRACE = {}
PLANES = ("mag", "filt", "open", "out")


def standin_opening(image, **kwargs):
    assert image.dtype == np.float32 and image.ndim == 2 and kwargs == dict(area_threshold=64, connectivity=1), (image.dtype, image.shape, kwargs)
    TRACE["filt"] = image.copy()
    return skr_scipy.area_opening(image, **kwargs)


def standin_closing(image, **kwargs):
    assert image.dtype == np.float32 and image.ndim == 2 and kwargs == dict(area_threshold=64, connectivity=1), (image.dtype, image.shape, kwargs)
    TRACE["open"] = image.copy()
    return skr_scipy.area_closing(image, **kwargs)


def reference_skrgan():
    sk, mor = types.ModuleType("skimage"), types.ModuleType("skimage.morphology")
    mor.area_opening, mor.area_closing = standin_opening, standin_closing
    sk.morphology = mor
    sys.modules["skimage"], sys.modules["skimage.morphology"] = sk, mor
    spec = importlib.util.spec_from_file_location("reference_skrgan", os.path.join(REF, "models", "skrgan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    scipy_gaussian = mod.gaussian_filter

    def recording_gaussian(image, sigma):
        TRACE["mag"] = image.copy()
        return scipy_gaussian(image, sigma=sigma)

    mod.gaussian_filter = recording_gaussian
    return mod.SkrGAN


def sha(plane):
    """signed zeros and the sign and payload of a NaN are not part of the contract"""
    return hashlib.sha256(np.ascontiguousarray(np.where(np.isnan(plane), np.float32(np.nan), plane + np.float32(0.0))).tobytes()).hexdigest()


def case(SkrGAN, name, img, step, full_out=False):
    TRACE.clear()
    t = torch.from_numpy(np.ascontiguousarray(img))[None, None]
    with np.errstate(invalid="ignore"):
        out = SkrGAN()(t)
    assert out.dtype == torch.float32 and out.shape == t.shape
    TRACE["out"] = out.numpy()[0, 0]
    assert all(TRACE[k].dtype == np.float32 and TRACE[k].shape == img.shape for k in PLANES)
    d = {f"{name}_step": np.int64(step), f"{name}_sha": np.array([sha(TRACE[k]) for k in PLANES], dtype="S64")}
    for k in PLANES:
        d[f"{name}_{k}"] = TRACE[k].copy() if (k == "out" and full_out) else TRACE[k][::step, ::step].copy()
    changed = [int((TRACE["filt"] != skr_scipy.area_opening(TRACE["filt"], 64)).sum()), int((TRACE["open"] != skr_scipy.area_closing(TRACE["open"], 64)).sum())]
    print(f"{name}: {img.shape} nan {int(np.isnan(TRACE['out']).sum())} pixels changed by opening / closing {changed} out mean {TRACE['out'].mean():.6f}")
    return d, TRACE["out"].copy()


def check_threshold(name, out, threshold, min_size):
    lab, n = ndi.label(out > threshold)        # connectivity 1, as RemoveSmallObjects
    kept = int((np.bincount(lab.ravel())[1:] >= min_size).sum())
    print(f"  {name} at {threshold}: {kept} of {n} objects kept (min_size {min_size})")
    assert kept >= 1, (name, threshold, kept)


def main():
    from test_oof import CASES
    print("stand-in opening equals the definition on", skr_scipy.self_check(), "planes")
    SkrGAN = reference_skrgan()
    rng = np.random.default_rng(20261021)
    steps = np.repeat(np.repeat(rng.integers(0, 6, (7, 9)), 3, axis=0), 3, axis=1)[:20, :26] * 51
    tiny = {"r8x8": rng.integers(0, 256, (8, 8), dtype=np.uint8), "r9x8": rng.integers(0, 256, (9, 8), dtype=np.uint8),
            "r12x11": rng.integers(0, 256, (12, 11), dtype=np.uint8), "r20x23": rng.integers(0, 256, (20, 23), dtype=np.uint8),
            "steps": steps.astype(np.uint8)}

    _, out = case(SkrGAN, "const", np.full((9, 9), np.float32(9 / 255)), 1)
    assert np.isnan(out).all()

    arrays = {"w_sigma2": _gaussian_kernel1d(2.0, 0, 8)}
    for name, u8 in tiny.items():
        d, out = case(SkrGAN, name, u8.astype(np.float32) / np.float32(255), 1)
        assert np.isnan(out).all() == (name in ("r8x8", "r9x8", "r12x11")) and np.isnan(out).all() == np.isnan(out).any()
        arrays.update(d)
        arrays[f"{name}_u8"] = u8
    for name, step, full_out in (("odd", 2, False), ("even", 1, True), ("octa", 4, True), ("crop", 8, False), ("full", 16, False)):
        d, out = case(SkrGAN, name, CASES[name]["img"], step, full_out)
        assert not np.isnan(out).any()
        arrays.update(d)
        if full_out:
            check_threshold(name, out, 0.5, 31)
            check_threshold(name, out, 0.5, 5)
    arrays["names"] = np.array(sorted(tiny) + ["odd", "even", "octa", "crop", "full"], dtype="S16")
    write_npz(os.path.join(GOLDEN, "skrgan_golden.npz"), arrays)


if __name__ == "__main__":
    main()
