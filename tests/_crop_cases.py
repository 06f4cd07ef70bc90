"""Shared by tests/test_crop.py (CPU tensors) and tests/test_crop_gpu.py (device tensors): the recorded calls of the reference's own
RandCropOrPadd (tests/golden/crop_golden.npz, written by tools/make_golden_crop.py) replayed through this repository's class."""
import functools
import os
import random

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["crop", "pad_f32", "pad_u8", "prob", "one", "range"]


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "crop_golden.npz"))
    return {k: g[k] for k in g.files}


def transform(name):
    from octa_autosegmentation_amd.data import data_transforms as T
    prob, lo, hi = golden()[f"{name}_args"].tolist()
    return T.RandCropOrPadd(["image", "label"], prob=prob, min_factor=lo, max_factor=hi)


def check_case(name, device):
    """Every recorded call of case `name` on tensors of `device`: values, dtype, shape and device of both outputs bit for bit, and the
    global `random` stream at the recorded position afterwards."""
    g = golden()
    t = transform(name)
    img, lab = (torch.from_numpy(g[f"{name}_in_{k}"].copy()).to(device) for k in ("image", "label"))
    random.seed(int(g[f"{name}_seed"]))
    shapes = set()
    for c in range(int(g[f"{name}_calls"])):
        d = t({"image": img.clone(), "label": lab.clone()})
        for k in ("image", "label"):
            want = g[f"{name}_out{c}_{k}"]
            got = d[k]
            assert got.device.type == torch.device(device).type
            assert got.cpu().numpy().dtype == want.dtype and tuple(got.shape) == want.shape, (name, c, k, got.dtype, tuple(got.shape))
            assert np.array_equal(got.cpu().numpy(), want), (name, c, k)
        shapes.add(tuple(d["image"].shape))
    assert random.random() == float(g[f"{name}_after"]), name
    return shapes
