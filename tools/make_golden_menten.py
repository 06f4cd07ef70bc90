"""tools/make_golden_menten.py -- generates tests/golden/menten_golden.npz: outputs of the reference's OWN Menten-augmentation classes
(data/data_transforms.py:44-325 BinomialVesselNoised, AddVitreousFloater, AddMotionArtifact, MentenAugmentationd) on seeded inputs.

Runs ONLY in the build container: imports /root/reference/data/data_transforms.py with its absent dependencies mocked (monai, the model
files; `monai.transforms.MapTransform` is given MONAI's documented minimal behaviour) and with this package's restatement of
skimage.draw.line (data/menten.py draw_line) injected as `skimage.draw.line` -- skimage is not installed, parity with it is unpinned.
The fixture stores inputs, seeds, constructor arguments and outputs, and after every call ONE further np.random.uniform(), which pins
where the reference's random stream ends. The archive is written with fixed zip timestamps: re-running rewrites it byte for byte."""
import io
import os
import sys
import types
import zipfile
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
OUT = os.path.join(ROOT, "tests", "golden", "menten_golden.npz")
sys.path.insert(0, ROOT)
from octa_autosegmentation_amd.data import menten  # noqa: E402


def image(shape, k, dtype=np.float32):
    n = int(np.prod(shape))
    v = 0.5 + 0.5 * np.sin(np.arange(n, dtype=np.float64) * 0.0137 * (k + 1) + np.arange(n, dtype=np.float64) ** 2 * 1e-7)
    return torch.from_numpy(v.astype(dtype)).reshape(shape)


def label(h, w):
    """Sparse binary pattern (thin oblique and vertical lines): distinct rows and columns, compresses well."""
    yy, xx = np.mgrid[0:h, 0:w]
    return torch.from_numpy((((3 * xx + 5 * yy) % 41 == 0) | ((xx % 29 == 7) & (yy % 3 != 0))).astype(np.float32)).reshape(1, h, w)


def load_reference():
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
    for m in ["monai", "monai.config", "monai.transforms", "monai.data", "monai.losses", "monai.networks", "monai.networks.nets", "skimage",
              "skimage.filters", "skimage.morphology", "nibabel", "prettytable", "natsort", "torchvision", "torchvision.transforms",
              "torchvision.transforms.functional", "models.networks", "models.noise_model", "matplotlib", "matplotlib.pyplot", "matplotlib.figure",
              "matplotlib.collections", "matplotlib.backends", "matplotlib.backends.backend_agg"]:
        sys.modules.setdefault(m, MagicMock())
    sys.modules["monai"] = monai
    sys.modules["monai.transforms"] = monai.transforms
    draw = types.ModuleType("skimage.draw")
    draw.line = menten.draw_line
    sys.modules["skimage.draw"] = draw
    import importlib
    return importlib.import_module("data.data_transforms")


def first_seed(start, accept):
    s = start
    while not accept(s):
        s += 1
    return s


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
    ref = load_reference()
    out = {}

    # BinomialVesselNoised: 64x64 with r = 20 (all five rings inside; (12, 16) from the centre lies exactly on the outermost), 40x56 with r = 18
    for k, (shape, r, dtype, kw) in enumerate((((1, 64, 64), 20, np.float32, {}), ((1, 40, 56), 18, np.float64, dict(vessel_noise_scaling=0.8, vessel_noise_blur=1.5)))):
        img = image(shape, k + 1, dtype)
        np.random.seed(400 + k)
        res = ref.BinomialVesselNoised(["image"], r=r, **kw)({"image": img.clone()})["image"]
        out[f"vessel_{k}_in"], out[f"vessel_{k}_out"], out[f"vessel_{k}_next"] = img.numpy(), res.numpy(), np.random.uniform()
        out[f"vessel_{k}_args"] = np.array([kw.get("vessel_noise_scaling", 0.5), kw.get("vessel_noise_blur", 1.0), r], dtype=np.float64)
        out[f"vessel_{k}_seed"] = np.int64(400 + k)

    # AddVitreousFloater
    def walk(seed, n):
        np.random.seed(seed)
        return menten.floater_draws(n, n, 1.0)[0]

    inside = lambda n: (lambda s: bool(np.all((walk(s, n) >= 0) & (walk(s, n) < n))))
    cases = [("floater_0", (1, 48, 48), first_seed(500, inside(48)), 1.0, np.float64),
             ("floater_1", (1, 32, 32), 501, 1.0, np.float64),                                         # smaller than the blur radius (40)
             ("floater_2", (1, 48, 48), first_seed(500, lambda s: not inside(48)(s)), 1.0, np.float32),  # the walk leaves the image
             ("floater_3", (1, 48, 48), first_seed(500, lambda s: np.random.RandomState(s).uniform() >= 0.1), 0.1, np.float32)]   # nothing happens
    for k, (name, shape, seed, chance, dtype) in enumerate(cases):
        img = image(shape, k + 3, dtype)
        np.random.seed(seed)
        res = ref.AddVitreousFloater(["image"], floater_chance=chance)({"image": img.clone()})["image"]
        out[f"{name}_in"], out[f"{name}_out"], out[f"{name}_next"] = img.numpy(), res.numpy(), np.random.uniform()
        out[f"{name}_seed"], out[f"{name}_chance"] = np.int64(seed), np.float64(chance)
    assert np.array_equal(out["floater_3_in"], out["floater_3_out"]) and out["floater_3_out"].dtype == np.float32
    img = image((1, 40, 56), 9, np.float64)                                                             # the mask is allocated (W, H): ValueError
    np.random.seed(510)
    try:
        ref.AddVitreousFloater(["image"], floater_chance=1.0)({"image": img.clone()})
        raise AssertionError("the reference should have raised")
    except ValueError as e:
        print("floater_4:", e)
    out["floater_4_in"], out["floater_4_next"], out["floater_4_seed"], out["floater_4_chance"] = img.numpy(), np.random.uniform(), np.int64(510), np.float64(1.0)

    # AddMotionArtifact: 48x48 image / 192x192 label; seeds such that every kind, a shear of 0, two cuts in one call and zero cuts all occur
    def cuts_of(seed):
        np.random.seed(seed)
        return menten.motion_draws(48, 48, {'shear': 0.3, 'stretch': 0.3, 'buckle': 0.3, 'whiteout': 0.1})

    wants = [("zero cuts", lambda c: len(c) == 0), ("shear of 0", lambda c: any(k == "shear" and a == 0 for k, _, a, _ in c)),
             ("shear", lambda c: any(k == "shear" and a > 0 for k, _, a, _ in c)), ("stretch", lambda c: any(k == "stretch" for k, *_ in c)),
             ("buckle", lambda c: any(k == "buckle" for k, *_ in c)), ("whiteout", lambda c: any(k == "whiteout" for k, *_ in c)),
             ("two cuts", lambda c: len(c) == 2), ("whiteout then another cut", lambda c: len(c) == 2 and c[0][0] == "whiteout" and c[1][0] != "whiteout"),
             ("two cuts of different kinds without whiteout", lambda c: len(c) == 2 and c[0][0] != c[1][0] and "whiteout" not in (c[0][0], c[1][0]))]
    seeds = []
    for what, pred in wants:
        s = first_seed(600, lambda s: pred(cuts_of(s)))
        print(f"motion: {what}: seed {s}: {[(k, p, a) for k, p, a, _ in cuts_of(s)]}")
        if s not in seeds:
            seeds.append(s)
    img, gt = image((1, 48, 48), 11, np.float64), label(192, 192)
    out["motion_in"], out["motion_gt"], out["motion_seeds"] = img.numpy(), gt.numpy(), np.array(seeds, dtype=np.int64)
    for s in seeds:
        out[f"motion_{s}_kinds"] = np.array([f"{k}:{p}:{a}" for k, p, a, _ in cuts_of(s)], dtype="U32")
        np.random.seed(s)
        d = ref.AddMotionArtifact("image", "label")({"image": img.clone(), "label": gt.clone()})
        out[f"motion_{s}_out"], out[f"motion_{s}_gt"], out[f"motion_{s}_next"] = d["image"].numpy(), d["label"].numpy(), np.random.uniform()

    # MentenAugmentationd on the 48 / 192 pair (float32 image, as the loader hands it over); a seed with a floater and at least one cut
    def full(seed):
        np.random.seed(seed)
        menten.vessel_noise_draws((48, 48))
        return menten.floater_draws(48, 48) is not None and len(menten.motion_draws(48, 48, {'shear': 0.3, 'stretch': 0.3, 'buckle': 0.3, 'whiteout': 0.1})) > 0

    seed = first_seed(700, full)
    img = image((1, 48, 48), 13, np.float32)
    np.random.seed(seed)
    d = ref.MentenAugmentationd("image", "label")({"image": img.clone(), "label": gt.clone()})
    out["menten_in"], out["menten_seed"] = img.numpy(), np.int64(seed)
    out["menten_out"], out["menten_gt"], out["menten_next"] = d["image"].numpy(), d["label"].numpy(), np.random.uniform()

    save_deterministic(OUT, out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes", {k: (v.shape, v.dtype) for k, v in np.load(OUT).items()})


if __name__ == "__main__":
    main()
