"""Shared by tests/test_noise_model.py (CPU) and tests/test_noise_model_gpu.py: the fixture of the reference's own NoiseModeld
(tests/golden/noise_model_golden.npz, written by tools/make_golden_noise_model.py) and the float32 / float64 torch evaluation of the noise
model's formula."""
import functools
import os
import random

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAMBDAS = ("lambda_delta", "lambda_speckle", "lambda_gamma")


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "noise_model_golden.npz"))


def cases():
    return [str(c) for c in golden()["cases"]]


def run_case(name, device):
    """The fixture's protocol on this package's NoiseModeld: seed, one instance, `calls` calls, one torch.rand(()) after each.
    -> [(output tensor, next draw, sample dict)] per call."""
    from octa_autosegmentation_amd.data import data_transforms as T
    g = golden()
    img, bg = torch.from_numpy(g[f"{name}_in"].copy()).to(device), torch.from_numpy(g[f"{name}_background"].copy()).to(device)
    torch.manual_seed(int(g[f"{name}_seed"]))
    random.seed(int(g[f"{name}_seed"]))
    t = T.NoiseModeld(["image"], **dict(zip(LAMBDAS, (float(v) for v in g[f"{name}_lambdas"]))))
    res = []
    for _ in range(int(g[f"{name}_calls"])):
        d = t({"image": img, "background": bg})
        res.append((d["image"], np.float32(torch.rand(()).item()), d))
    return res


def evaluate(img, bg, grids, delta, n, lambdas, dtype):
    """The noise model's formula by torch on the CPU in `dtype`, Delta and N given: img, bg, delta, n [B,H,W]; grids [B,5,gh,gw].
    -> (out [B,H,W], maps [B,5,H,W] with the four shape maps clamped as the sampler gets them, raw bicubic maps [B,5,H,W])."""
    ld, ls, lg = lambdas
    img, bg, grids, delta, n = (t.detach().cpu().to(dtype) for t in (img, bg, grids, delta, n))
    g5 = torch.cat([grids[:, :4], torch.clamp(grids[:, 4:], 0, 1) * (2 * lg) + (1 - lg)], dim=1)
    raw = F.interpolate(g5, img.shape[-2:], mode="bicubic")
    maps = torch.cat([torch.clamp(raw[:, :4], min=1e-3), raw[:, 4:]], dim=1)
    x = torch.maximum(img, bg * ld * delta)
    x = x * (ls * n + (1 - ls))
    return torch.pow(x + 1e-6, maps[:, 4]), maps, raw
