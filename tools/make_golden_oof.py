"""tools/make_golden_oof.py -- generates tests/golden/oof_golden.npz and tests/golden/oof_golden_304.npz: the reference's OWN
OOF filter (models/oof.py: numpy FFTs, scipy's besselj, np.linalg.eigvals) on five inputs (models/oof.py of this repository,
csrc/oof.hip).

Runs ONLY in the build container: imports /root/reference/models/oof.py at run time (nothing of it is committed). Every input
is stored exactly, as uint8 (bit-packed for binary masks) plus the rule img = u8.astype(float32) / float32(div); for each case
the fixture holds the reference's final output OOF()(img) and its pre-normalisation response _compute_oof(img * 255), at every
pixel or at every `step`-th pixel of both axes, and max |response| (the scale of the response tolerance):
  odd   91 x 97 random uint8 (div 255), full;
  even  64 x 48 random uint8 holding 0 and 255 (div 255), full;
  octa  the first 304 x 304 OCTA image of datasets/images (div = its maximum, 254: what ScaleIntensityd makes of the PNG; own
        file, oof_golden_304.npz, to keep each file below 1 MiB), output full, response every 4th pixel;
  crop  a 400 x 400 crop of the first datasets/labels mask (div 1), every 4th pixel;
  full  that whole 1216 x 1216 mask (div 1), every 8th pixel, plus the exact max, min and sum of the output.
Re-running it rewrites both files byte for byte."""
import glob
import importlib.util
import os

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "..", "tests", "golden")
REF = "/root/reference"


def reference_oof():
    spec = importlib.util.spec_from_file_location("reference_oof", os.path.join(REF, "models", "oof.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.OOF


def case(OOF, name, u8, div, step, packed=False):
    img = u8.astype(np.float32) / np.float32(div)
    f = OOF()
    out = f(torch.from_numpy(img)[None, None]).numpy()[0, 0]
    raw = OOF()._compute_oof(img * 255, f.radii)
    assert out.dtype == np.float64 and raw.dtype == np.float64
    d = {f"{name}_shape": np.array(u8.shape, np.int64), f"{name}_div": np.float32(div), f"{name}_step": np.int64(step),
         f"{name}_raw_absmax": np.float64(np.abs(raw).max())}
    if packed:
        assert set(np.unique(u8)) <= {0, 1}
        d[f"{name}_bits"] = np.packbits(u8.astype(np.uint8).reshape(-1))
    else:
        d[f"{name}_u8"] = u8
    return d, out, raw


def main():
    OOF = reference_oof()
    rng = np.random.default_rng(20261016)
    small = {}

    odd = rng.integers(0, 256, size=(91, 97), dtype=np.uint8)
    d, out, raw = case(OOF, "odd", odd, 255, 1)
    small.update(d, odd_out=out, odd_raw=raw)

    even = rng.integers(0, 256, size=(64, 48), dtype=np.uint8)
    even[0, 0], even[-1, -1] = 0, 255
    d, out, raw = case(OOF, "even", even, 255, 1)
    small.update(d, even_out=out, even_raw=raw)

    label = np.asarray(Image.open(sorted(glob.glob(os.path.join(REF, "datasets", "labels", "*.png")))[0])).astype(np.uint8)
    assert label.shape == (1216, 1216)
    crop = np.ascontiguousarray(label[400:800, 300:700])
    d, out, raw = case(OOF, "crop", crop, 1, 4, packed=True)
    small.update(d, crop_out=out[::4, ::4].copy(), crop_raw=raw[::4, ::4].copy())

    d, out, raw = case(OOF, "full", label, 1, 8, packed=True)
    small.update(d, full_out=out[::8, ::8].copy(), full_raw=raw[::8, ::8].copy(), full_out_max=np.float64(out.max()),
                 full_out_min=np.float64(out.min()), full_out_sum=np.float64(out.sum()))
    np.savez_compressed(os.path.join(GOLDEN, "oof_golden.npz"), **small)

    octa = np.asarray(Image.open(sorted(glob.glob(os.path.join(REF, "datasets", "images", "*.png")))[0]).convert("L"))
    assert octa.shape == (304, 304) and octa.min() == 0
    d, out, raw = case(OOF, "octa", octa, int(octa.max()), 4)
    d.update(octa_out=out, octa_raw=raw[::4, ::4].copy())
    np.savez_compressed(os.path.join(GOLDEN, "oof_golden_304.npz"), **d)
    for f in ("oof_golden.npz", "oof_golden_304.npz"):
        print(f, os.path.getsize(os.path.join(GOLDEN, f)), "bytes")


if __name__ == "__main__":
    main()
