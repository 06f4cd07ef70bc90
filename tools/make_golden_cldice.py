"""tools/make_golden_cldice.py -- generates tests/golden/cldice_golden.npz: scores of the reference's OWN clDice (utils/cldice.py
clDice, utils/metrics.py ClDiceMetric and its nanmean aggregate) on small seeded maps.

Runs ONLY in the build container: imports /root/reference/utils/cldice.py and utils/metrics.py with their absent dependencies mocked
(monai) and with this package's restatement of the 2-D skeleton (utils/skeleton.py skeletonize_host, returned as bool like skimage's)
injected as `skimage.morphology.skeletonize` -- skimage is not installed, parity with it is unpinned. What the fixture pins is
everything AROUND the skeleton: the two overlap ratios with `v` multiplied by value, the harmonic mean, NaN for 0 / 0, the layer loop
and the nanmean. Float maps hold multiples of 1/4 only, so that the reference's sums in the maps' dtype are exact.
The archive is written with fixed zip timestamps: re-running rewrites it byte for byte."""
import os
import sys
import types
import warnings
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
OUT = os.path.join(ROOT, "tests", "golden", "cldice_golden.npz")
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from octa_autosegmentation_amd.utils.skeleton import skeletonize_host  # noqa: E402
from make_golden_menten import save_deterministic  # noqa: E402


def load_reference():
    sys.path.insert(0, "/root/reference")
    for m in ["monai", "monai.metrics", "skimage"]:
        sys.modules[m] = MagicMock()
    morph = types.ModuleType("skimage.morphology")
    morph.skeletonize = lambda image, **kw: skeletonize_host(image).astype(bool)
    sys.modules["skimage.morphology"] = morph
    import importlib
    return importlib.import_module("utils.cldice"), importlib.import_module("utils.metrics")


def vessels(h, w, k):
    """Thick oblique and vertical bands: a vessel-like binary pattern with junctions."""
    yy, xx = np.mgrid[0:h, 0:w]
    return (((3 * xx + (5 + k) * yy) % 37 < 9) | ((xx % (23 + k) < 5) & (yy % 11 != k))).astype(np.uint8)


def cases():
    rng = np.random.default_rng(2024)
    c = {}
    lab = vessels(64, 64, 0)
    c["similar"] = (np.roll(lab, 1, axis=1)[None], lab[None])                                     # uint8, shifted by one pixel
    c["rect"] = (vessels(40, 56, 2)[None].astype(np.float32), vessels(40, 56, 3)[None].astype(np.float32))
    c["emptypred"] = (np.zeros((1, 32, 48), np.float32), vessels(32, 48, 1)[None].astype(np.float32))     # tsens = 0 / 0
    c["emptylabel"] = (vessels(32, 48, 1)[None], np.zeros((1, 32, 48), np.uint8))                          # tprec = 0 / 0
    a, b = np.zeros((1, 48, 48), np.uint8), np.zeros((1, 48, 48), np.uint8)
    a[0, 4:20, 4:40], b[0, 28:44, 4:40] = 1, 1
    c["disjoint"] = (a, b)                                                                               # both ratios 0: 0 / 0
    soft = vessels(64, 64, 4) * rng.integers(1, 5, (64, 64)) / 4.0                                       # values 0.25 .. 1
    c["softpred"] = (soft[None].astype(np.float32), vessels(64, 64, 5)[None].astype(np.float32))
    c["softboth"] = ((vessels(33, 47, 6) * rng.integers(1, 9, (33, 47)) / 4.0)[None],                    # float64, values up to 2
                     (vessels(33, 47, 7) * rng.integers(1, 5, (33, 47)) / 4.0)[None])
    c["twolayer"] = (np.stack([vessels(48, 40, 8), np.zeros((48, 40), np.uint8)]).astype(np.float32),    # second layer: NaN
                     np.stack([vessels(48, 40, 9), vessels(48, 40, 10)]).astype(np.float32))
    return c


def main():
    cl, met = load_reference()
    out, names = {}, []
    metric = met.ClDiceMetric()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                   # 0 / 0 is the point of three cases
        for name, (pred, label) in cases().items():
            names.append(name)
            scores = np.array([cl.clDice(pred[k], label[k]) for k in range(len(pred))], dtype=np.float64)
            one = met.ClDiceMetric()
            one([torch.from_numpy(pred)], [torch.from_numpy(label)])
            assert np.array_equal(np.asarray(one.scores, dtype=np.float64), scores, equal_nan=True)
            metric([torch.from_numpy(pred)], [torch.from_numpy(label)])
            out[f"{name}_pred"], out[f"{name}_label"], out[f"{name}_scores"] = pred, label, scores
            print(name, pred.dtype, pred.shape, scores)
        out["aggregate"] = np.float64(metric.aggregate().item())
    out["names"] = np.array(names, dtype="U16")
    assert sum(int(np.isnan(out[f"{n}_scores"]).sum()) for n in names) == 4
    save_deterministic(OUT, out)
    print("aggregate", out["aggregate"], "wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
