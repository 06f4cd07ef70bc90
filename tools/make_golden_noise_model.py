"""tools/make_golden_noise_model.py -- generates tests/golden/noise_model_golden.npz: outputs of the reference's OWN noise model
(data/data_transforms.py:435-475 NoiseModeld -> models/noise_model.py NoiseModel, adversarial=False) on seeded inputs.

    python tools/make_golden_noise_model.py --reference /path/to/the/reference/checkout

Imports the reference's data/data_transforms.py with its absent dependencies mocked (monai, skimage, the network definitions;
`monai.transforms.MapTransform` is given MONAI's documented minimal behaviour) and its real models/noise_model.py, which needs torch only.
Per case the fixture holds the inputs, the torch seed, the constructor arguments, and for every recorded call of ONE instance: the output,
the five control grids the reference used in that call (read back from its parameters), and one further torch.rand(()) that pins where the
reference leaves torch's generator. Recording the first AND the second call pins that the first call draws its control points twice. For the
first call of the default cases the five bicubic maps are stored too, recomputed here from those grids with torch (float32, before the clamp).
Data only; the archive is written with fixed zip timestamps: re-running rewrites it byte for byte."""
import argparse
import importlib
import io
import os
import random
import sys
import zipfile
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden", "noise_model_golden.npz")

# name, shape, torch seed, recorded calls, constructor arguments
CASES = [("a", (1, 40, 56), 800, 2, {}),
         ("b", (1, 96, 128), 801, 2, {}),
         ("c", (1, 40, 56), 802, 1, dict(lambda_delta=0.8, lambda_speckle=0.5, lambda_gamma=0.2))]
LAMBDAS = ("lambda_delta", "lambda_speckle", "lambda_gamma")
DEFAULTS = dict(lambda_delta=1, lambda_speckle=0.7, lambda_gamma=0.3)


def image(shape, k):
    n = int(np.prod(shape))
    v = 0.5 + 0.5 * np.sin(np.arange(n, dtype=np.float64) * 0.0137 * (k + 1) + np.arange(n, dtype=np.float64) ** 2 * 1e-7)
    return torch.from_numpy(v.astype(np.float32)).reshape(shape)


def load_reference(path):
    sys.path.insert(0, path)
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
              "torchvision.transforms.functional", "models.networks", "matplotlib", "matplotlib.pyplot", "matplotlib.figure",
              "matplotlib.collections", "matplotlib.backends", "matplotlib.backends.backend_agg"]:
        sys.modules.setdefault(m, MagicMock())
    sys.modules["monai"] = monai
    sys.modules["monai.transforms"] = monai.transforms
    ref = importlib.import_module("data.data_transforms")
    assert type(ref.NoiseModel).__name__ != "MagicMock", "models/noise_model.py must be the reference's real module"
    return ref


def save_deterministic(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ref = load_reference(ap.parse_args().reference)
    out = {"cases": np.array([c[0] for c in CASES], dtype="U4")}
    for k, (name, shape, seed, calls, kw) in enumerate(CASES):
        img, bg = image(shape, k + 1), image(shape, k + 7).flip(-1) * 0.6
        out[f"{name}_in"], out[f"{name}_background"] = img.numpy().copy(), bg.numpy().copy()
        out[f"{name}_seed"], out[f"{name}_calls"] = np.int64(seed), np.int64(calls)
        out[f"{name}_lambdas"] = np.array([kw.get(l, DEFAULTS[l]) for l in LAMBDAS], dtype=np.float64)
        torch.manual_seed(seed)
        random.seed(seed)
        t = ref.NoiseModeld(["image"], **kw)
        for c in range(calls):
            d = t({"image": img.clone(), "background": bg.clone()})
            assert torch.equal(d["background"], bg) and d["image"].shape == shape and d["image"].dtype == torch.float32
            m = t.noise_model
            grids = torch.cat([m.vessel_noise.alpha_unbound, m.vessel_noise.beta_unbound, m.specle_noise.alpha_unbound, m.specle_noise.beta_unbound,
                               m.control_points_gamma], dim=1).detach()[0]
            out[f"{name}_{c}_out"], out[f"{name}_{c}_grids"] = d["image"].numpy().copy(), grids.numpy().copy()
            out[f"{name}_{c}_next"] = np.float32(torch.rand(()).item())
            if c == 0 and not kw:
                lg = DEFAULTS["lambda_gamma"]
                g5 = torch.cat([grids[:4], torch.clamp(grids[4:], 0, 1) * (2 * lg) + (1 - lg)])[None]
                maps = torch.nn.functional.interpolate(g5, shape[1:], mode="bicubic")[0]
                print(f"case {name}: bicubic shape maps span [{maps[:4].min().item():.3f}, {maps[:4].max().item():.3f}]")
                out[f"{name}_{c}_maps"] = maps.numpy().copy()
    assert min(out[f"{n}_0_maps"][:4].min() for n in ("a", "b")) < 1e-3, "no case exercises the clamp"
    save_deterministic(OUT, out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes", {k: (v.shape, v.dtype) for k, v in np.load(OUT).items()})


if __name__ == "__main__":
    main()
