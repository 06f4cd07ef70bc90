"""tools/make_golden_noise_model_at.py -- generates tests/golden/noise_model_at_golden.npz: seeded runs of the reference's OWN adversarial
augmentation loop (utils/losses.py ANTLoss around models/noise_model.py NoiseModel) on the CPU.

    python tools/make_golden_noise_model_at.py --reference /path/to/the/reference/checkout

Imports the reference's utils/losses.py with its absent dependencies mocked (monai, torchvision) and its real models/noise_model.py. Two things
are injected, because the reference needs packages that are not installed here:
  * torchvision.transforms.functional.rotate is replaced by this package's restatement (models/noise_model_at.py rotate_bilinear), so the
    fixture pins the loop AROUND the rotation, not the rotation against torchvision;
  * the GradScaler is a stand-in whose scale(v) is v * 65536, a new torch.cuda.amp.GradScaler's factor.
The network is a two-layer convolution whose weights are stored; the loss is this package's DiceBCELoss(sigmoid) on its torch path.
Per case: inputs, seeds, the Train.AT keys, the python-random draws in the order made, the five control grids as drawn and after each of the
three ascent steps, the three losses, the returned sample and label, and one further random.random() / torch.rand(()) that pin where both
generators are left. Data only; fixed zip timestamps."""
import argparse
import importlib
import os
import random
import sys
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
from make_golden_noise_model import image, save_deterministic  # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden", "noise_model_at_golden.npz")
CASES = [("full", 900, {}), ("crop", 901, dict(crop=[0.75, 0.75], alpha=0.002, lambda_gamma=0.2))]
IMAGE, LABEL = (2, 1, 32, 32), (2, 1, 48, 48)


def make_net(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3, padding=1), torch.nn.LeakyReLU(0.01), torch.nn.Conv2d(4, 1, 3, padding=1))


class Scaler:
    def scale(self, v):
        return v * 65536.0


def load_reference(path):
    sys.path.insert(0, path)
    for m in ["monai", "monai.losses", "torchvision", "torchvision.transforms", "torchvision.transforms.functional"]:
        sys.modules.setdefault(m, MagicMock())
    ref = importlib.import_module("utils.losses")
    assert type(ref.NoiseModel).__name__ != "MagicMock", "models/noise_model.py must be the reference's real module"
    from octa_autosegmentation_amd.models.noise_model_at import rotate_bilinear
    ref.rotate = lambda img, angle, interpolation=None: rotate_bilinear(img, angle)
    return ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ref = load_reference(ap.parse_args().reference)
    from octa_autosegmentation_amd.models.losses import DiceBCELoss
    out = {"cases": np.array([c[0] for c in CASES], dtype="U8")}
    for k, (name, seed, kw) in enumerate(CASES):
        x, bg = image(IMAGE, k + 1), image(IMAGE, k + 7).flip(-1) * 0.6
        y = (image(LABEL, k + 3) > 0.6).float() * image(LABEL, k + 4)              # values around the threshold too
        net = make_net(seed)
        for i, p in enumerate(net.parameters()):
            out[f"{name}_net_{i}"] = p.detach().numpy().copy()
        out[f"{name}_x"], out[f"{name}_background"], out[f"{name}_y"] = x.numpy().copy(), bg.numpy().copy(), y.numpy().copy()
        out[f"{name}_seed"] = np.int64(seed)
        out[f"{name}_at"] = np.array(repr(kw))
        torch.manual_seed(seed)
        random.seed(seed)
        at = ref.ANTLoss(Scaler(), DiceBCELoss(True), **kw)
        grids, inner = [], at._create_adversarial_sample

        def recorded(*a, **b):
            s = inner(*a, **b)
            m = at.noise_model
            grids.append(torch.cat([m.vessel_noise.alpha_unbound, m.vessel_noise.beta_unbound, m.specle_noise.alpha_unbound,
                                    m.specle_noise.beta_unbound, m.control_points_gamma], dim=1).detach().clone().numpy())
            return s

        at._create_adversarial_sample = recorded
        losses = []
        loss_fun = at.loss_fun
        at.loss_fun = lambda p, t: (losses.append(loss_fun(p, t)), losses[-1])[1]
        adv, y_crop = at(net, x.clone(), bg.clone(), y.clone())
        torch.autograd.set_detect_anomaly(False)
        assert len(grids) == 4 and not any(p.grad is not None for p in net.parameters()) and all(p.requires_grad for p in net.parameters())
        out[f"{name}_grids"] = np.stack(grids)
        out[f"{name}_losses"] = np.array([v.item() for v in losses], dtype=np.float32)
        out[f"{name}_adv"], out[f"{name}_label"] = adv.numpy().copy(), y_crop.numpy().copy()
        out[f"{name}_downsample_factor"] = np.array(at.downsample_factor, dtype=np.float64)
        out[f"{name}_rot_k"], out[f"{name}_rot_r"] = np.array(at.rot_k, dtype=np.int64), np.array(at.rot_r, dtype=np.float64)
        if "crop" in kw:
            out[f"{name}_h_crop"], out[f"{name}_w_crop"] = np.array(at.h_crop, dtype=np.int64), np.array(at.w_crop, dtype=np.int64)
        out[f"{name}_next_python"], out[f"{name}_next_torch"] = np.float64(random.random()), np.float32(torch.rand(()).item())
        steps = [float(np.abs(grids[i + 1] - grids[i]).max()) for i in range(3)]
        print(f"case {name}: losses {out[f'{name}_losses']}, largest grid step per iteration {steps}, sample {adv.shape}, label {y_crop.shape}")
        assert min(steps) > 0
    save_deterministic(OUT, out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
