"""Shared by tests/test_menten.py and tests/test_menten_gpu.py: the cases of tests/golden/menten_golden.npz (tools/make_golden_menten.py) and
one runner that feeds them to this package's transforms on a given device."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "menten_golden.npz")
_cache = {}


def golden():
    if "g" not in _cache:
        with np.load(GOLDEN) as g:
            _cache["g"] = {k: g[k] for k in g.files}
        for v in _cache["g"].values():
            v.setflags(write=False)
    return _cache["g"]


def vessel_cases():
    return [0, 1]


def floater_cases():
    return [0, 1, 2, 3]


def motion_seeds():
    return [int(s) for s in golden()["motion_seeds"]]


def run_vessel(k, device):
    """-> (output tensor, the draw that follows, the input tensor as handed over, a pristine copy of it)"""
    from octa_autosegmentation_amd.data import data_transforms as T
    g = golden()
    scaling, blur, r = g[f"vessel_{k}_args"]
    x = torch.from_numpy(g[f"vessel_{k}_in"].copy()).to(device)
    keep = x.clone()
    np.random.seed(int(g[f"vessel_{k}_seed"]))
    out = T.BinomialVesselNoised(["image"], vessel_noise_scaling=float(scaling), vessel_noise_blur=float(blur), r=int(r))({"image": x})["image"]
    return out, np.random.uniform(), x, keep


def run_floater(k, device):
    from octa_autosegmentation_amd.data import data_transforms as T
    g = golden()
    x = torch.from_numpy(g[f"floater_{k}_in"].copy()).to(device)
    keep = x.clone()
    np.random.seed(int(g[f"floater_{k}_seed"]))
    out = T.AddVitreousFloater(["image"], floater_chance=float(g[f"floater_{k}_chance"]))({"image": x})["image"]
    return out, np.random.uniform(), x, keep


def run_motion(seed, device):
    from octa_autosegmentation_amd.data import data_transforms as T
    g = golden()
    x, y = torch.from_numpy(g["motion_in"].copy()).to(device), torch.from_numpy(g["motion_gt"].copy()).to(device)
    keep = (x.clone(), y.clone())
    np.random.seed(seed)
    d = T.AddMotionArtifact("image", "label")({"image": x, "label": y})
    return d["image"], d["label"], np.random.uniform(), (x, y), keep


def run_menten(device):
    from octa_autosegmentation_amd.data import data_transforms as T
    g = golden()
    x, y = torch.from_numpy(g["menten_in"].copy()).to(device), torch.from_numpy(g["motion_gt"].copy()).to(device)
    np.random.seed(int(g["menten_seed"]))
    d = T.MentenAugmentationd("image", "label")({"image": x, "label": y})
    return d["image"], d["label"], np.random.uniform()
