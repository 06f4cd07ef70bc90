"""tools/time_menten.py -- per-sample cost of the Menten et al. augmentation on the GPU, at the training configs' sizes (image 304x304,
label 1216x1216): for each of BinomialVesselNoised, AddVitreousFloater (floater_chance 1: the expensive branch) and AddMotionArtifact the
milliseconds of the host draws (numpy's global stream, data/menten.py) and of the device part (uploads + kernels of csrc/menten.hip, timed
to a device synchronise), and beside them the same two figures for SpeckleBrightnesd + AddRandomBackgroundNoised, the noise model's
per-sample transforms, in the same run. Needs a GPU.   python tools/time_menten.py [--reps 50]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from octa_autosegmentation_amd.data import data_transforms as T  # noqa: E402
from octa_autosegmentation_amd.data import gpu_augment, menten  # noqa: E402


def timed(fn, reps):
    """(mean host-draw ms, mean device ms) of fn() -> (draw seconds, thunk that enqueues the device part)."""
    draw = dev = 0.0
    for i in range(reps + 3):
        t0 = time.perf_counter()
        thunk = fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        thunk()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if i >= 3:                   # three warm-up rounds: code objects, allocator
            draw += t1 - t0
            dev += t3 - t2
    return 1e3 * draw / reps, 1e3 * dev / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_menten.py measures on the GPU; none is visible")
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.RandomState(0)
    img32 = torch.from_numpy(rng.rand(1, 304, 304).astype(np.float32)).to(dev)
    img64 = img32.double()
    lab = torch.from_numpy((rng.rand(1, 1216, 1216) < 0.2).astype(np.float32)).to(dev)
    bg = torch.from_numpy(rng.rand(1, 304, 304).astype(np.float32)).to(dev)
    arts = {'shear': 0.3, 'stretch': 0.3, 'buckle': 0.3, 'whiteout': 0.1}
    np.random.seed(0); torch.manual_seed(0)

    def vessel():
        bern, q = menten.vessel_noise_draws((304, 304))
        return lambda: gpu_augment.menten_vessel_noise(img32, torch.from_numpy(bern).to(dev)[None], torch.from_numpy(q).to(dev)[None], 1.0, 0.5, 48)

    def floater():
        pts, _, dil = menten.floater_draws(304, 304, 1.0)
        return lambda: gpu_augment.menten_floater(img64, [pts], [dil])

    def motion():
        cuts = menten.motion_draws(304, 304, arts)
        t1, white = menten.fold_cuts(304, 304, cuts, 1)
        t4 = menten.fold_cuts(304, 304, cuts, 4)[0]
        return lambda: (gpu_augment.menten_motion(img64, t1, white), gpu_augment.menten_motion(lab, t4))

    def noise_model():
        c = torch.rand((1, 1, 9, 9)) * 0.5 + 0.5
        u = torch.rand((1, 304, 304))
        speckle = np.random.uniform(0, 1, (1, 304, 304))
        return lambda: gpu_augment.background_noise(gpu_augment.speckle_brightness(img32, c.reshape(1, 9, 9).to(dev), u.to(dev)), bg,
                                                    torch.from_numpy(speckle).to(dev))

    print(f"per 304x304 / 1216x1216 sample, mean of {a.reps} (ms): host draws | device part (uploads + kernels, synchronised)")
    total = [0.0, 0.0]
    for name, fn in (("BinomialVesselNoised", vessel), ("AddVitreousFloater (chance 1)", floater), ("AddMotionArtifact", motion)):
        d, k = timed(fn, a.reps)
        total[0] += d; total[1] += k
        print(f"  {name:32s} {d:8.3f} | {k:8.3f}")
    print(f"  {'sum of the three':32s} {total[0]:8.3f} | {total[1]:8.3f}")
    d, k = timed(noise_model, a.reps)
    print(f"  {'Speckle + BackgroundNoise':32s} {d:8.3f} | {k:8.3f}")
    # the transform itself, as the loader calls it (draws, uploads, kernels, default floater chance), wall clock to a synchronise
    t = T.MentenAugmentationd("image", "label")
    for i in range(a.reps + 3):
        if i == 3:
            torch.cuda.synchronize(); t0 = time.perf_counter()
        t({"image": img32, "label": lab})
    torch.cuda.synchronize()
    print(f"  MentenAugmentationd end to end   {1e3 * (time.perf_counter() - t0) / a.reps:8.3f} ms per sample")


if __name__ == "__main__":
    main()
