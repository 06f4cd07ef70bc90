"""tools/make_golden_crop.py -- generates tests/golden/crop_golden.npz: outputs of the reference's OWN RandCropOrPadd
(data/data_transforms.py:543-585) on seeded inputs.

Runs ONLY in the build container: imports /root/reference/data/data_transforms.py with its absent dependencies mocked, as
tools/make_golden_noise.py does (`monai.transforms.MapTransform` is given MONAI's documented minimal behaviour: `keys` as a tuple and
`allow_missing_keys`). Per case the fixture stores the seed given to `random.seed`, the constructor arguments, the input arrays, the
outputs and the value of `random.random()` taken right after the call(s), which pins the position of the global stream. The 1216^2 case
is stored as shapes and offsets only (the input is an index ramp, so the window's first element names its offsets)."""
import os
import random
import sys
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden", "crop_golden.npz")


def image(shape, k, dtype=np.float32):
    n = int(np.prod(shape))
    v = 0.5 + 0.5 * np.sin(np.arange(n, dtype=np.float64) * 0.0137 * (k + 1) + np.arange(n, dtype=np.float64) ** 2 * 1e-7)
    if dtype == np.uint8:
        return torch.from_numpy((v * 255).astype(np.uint8)).reshape(shape)
    return torch.from_numpy(v.astype(np.float32)).reshape(shape)


def reference_module():
    sys.path.insert(0, "/root/reference")
    monai = MagicMock()

    class MapTransform:
        def __init__(self, keys, allow_missing_keys=False):
            self.keys = (keys,) if isinstance(keys, str) else tuple(keys)
            self.allow_missing_keys = allow_missing_keys

    class Randomizable:
        pass

    class Transform:
        pass

    monai.transforms.MapTransform, monai.transforms.Randomizable, monai.transforms.Transform = MapTransform, Randomizable, Transform
    monai.transforms.__all__ = []
    for m in ["monai", "monai.config", "monai.transforms", "monai.data", "monai.losses", "monai.networks", "monai.networks.nets", "skimage", "skimage.draw",
              "skimage.filters", "skimage.morphology", "nibabel", "prettytable", "natsort", "torchvision", "torchvision.transforms",
              "torchvision.transforms.functional", "models.networks", "models.noise_model", "matplotlib", "matplotlib.pyplot", "matplotlib.figure",
              "matplotlib.collections", "matplotlib.backends", "matplotlib.backends.backend_agg"]:
        sys.modules.setdefault(m, MagicMock())
    sys.modules["monai"] = monai
    sys.modules["monai.transforms"] = monai.transforms
    import importlib
    return importlib.import_module("data.data_transforms")


# name -> (seed, (prob, min_factor, max_factor), input dtype, number of consecutive calls); inputs: image(k=1) and label(k=2) of [1, 24, 31]
CASES = {
    "crop": (11, (1, 0.5, 0.5), np.float32, 1),
    "pad_f32": (12, (1, 1.3, 1.3), np.float32, 1),
    "pad_u8": (13, (1, 1.3, 1.3), np.uint8, 1),
    "prob": (14, (0.3, 0.5, 0.5), np.float32, 8),
    "one": (15, (1, 1, 1), np.float32, 1),
    "range": (16, (1, 0.4, 0.9), np.float32, 3),
}
SHAPE = (1, 24, 31)


def main():
    ref = reference_module()
    out = {}
    for name, (seed, (prob, lo, hi), dtype, calls) in CASES.items():
        img, lab = image(SHAPE, 1, dtype), image(SHAPE, 2, dtype)
        out[f"{name}_seed"] = np.int64(seed)
        out[f"{name}_args"] = np.array([prob, lo, hi], dtype=np.float64)
        out[f"{name}_calls"] = np.int64(calls)
        out[f"{name}_in_image"], out[f"{name}_in_label"] = img.numpy().copy(), lab.numpy().copy()
        t = ref.RandCropOrPadd(["image", "label"], prob=prob, min_factor=lo, max_factor=hi)
        random.seed(seed)
        for c in range(calls):
            d = t({"image": img.clone(), "label": lab.clone()})
            out[f"{name}_out{c}_image"], out[f"{name}_out{c}_label"] = d["image"].numpy().copy(), d["label"].numpy().copy()
        out[f"{name}_after"] = np.float64(random.random())
    applied = [out[f"prob_out{c}_image"].shape != SHAPE for c in range(8)]
    assert any(applied) and not all(applied), applied          # the prob case mixes applied and not applied calls
    # the Giarratano set-up's sizes: 1216 -> 360, shapes and offsets only. Pixel (r, c) of the ramp holds r * 1216 + c (exact in float32 up to 2^24)
    ramp = torch.arange(1216 * 1216, dtype=torch.float32).reshape(1, 1216, 1216)
    t = ref.RandCropOrPadd(["image", "label"], prob=1, min_factor=0.2965, max_factor=0.2965)
    random.seed(17)
    shapes, offsets = [], []
    for c in range(4):
        d = t({"image": ramp, "label": ramp})
        first = int(d["image"][0, 0, 0].item())
        assert torch.equal(d["image"], d["label"])
        shapes.append(tuple(d["image"].shape))
        offsets.append((first // 1216, first % 1216))
    out["big_seed"], out["big_args"] = np.int64(17), np.array([1, 0.2965, 0.2965], dtype=np.float64)
    out["big_shapes"], out["big_offsets"] = np.array(shapes, dtype=np.int64), np.array(offsets, dtype=np.int64)
    out["big_after"] = np.float64(random.random())
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes", {k: (v.shape, v.dtype) for k, v in out.items()})


if __name__ == "__main__":
    main()
