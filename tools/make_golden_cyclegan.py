"""tools/make_golden_cyclegan.py -- generates tests/golden/cyclegan_golden.npz: the reference's OWN CycleGAN update
(models/cycle_gan.py:147-248 driven through BaseModelABC.initialize_model_and_optimizer) and its ImagePool (:287-336) recorded on
seeded CPU inputs, so that a wrong detach, a wrong pairing of generator and discriminator, a pool queried in the wrong order or a
draw too many in this repository's models/cycle_gan.py fails a test.

Runs ONLY in the build container: imports /root/reference (read-only) with the stand-ins of tools/make_golden_ganseg.py (monai and the
other absent packages as MagicMock; generators and discriminators are the reference's own classes). All parameters come from the
closed form `he_weights` (a distinct salt per network), inputs from `image`: no weights travel.

Per variant FOUR consecutive steps at 2 x 1 x 32 x 32, `torch.manual_seed` and `random.seed` set once in front of them:
  bg        lambda_idt = 1,   pool_size = 2, batch with a `background` entry
  nobg      the same without `background` (pins the extra rand_like draw)
  idt05     lambda_idt = 0.5, pool_size = 0, with `background`
With batch 2 and pool_size 2 step 1 fills the pools and steps 2 - 4 make the `random` draws; the `random` seed is searched from 0 upwards until
both pools exchange at least once, and recorded. Recorded per variant: the nine losses and the four networks' gradient norms after
every step, float64 checksums of every network's parameters after the last step, and `random.random()` / `torch.rand(1)` drawn after
the last step (the stream positions).

Separately the reference's ImagePool alone: pool_size 3, 40 queries of batches of 3 constant planes that carry their serial number;
the returned serial numbers, the final pool and the stream position, with a seed at which at least one batch draws the same slot twice.
"""
import argparse
import os
import random
import sys
import warnings
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden", "cyclegan_golden.npz")
sys.path.insert(0, ROOT)
from tools.make_golden_ganseg import he_weights  # noqa: E402
from tools.make_golden_networks import image  # noqa: E402

TRAIN = {"lr": 2e-4, "epochs": 100, "epochs_decay": 0, "loss_criterionGAN": "LSGANLoss", "loss_criterionCycle": "L1Loss", "loss_criterionIdt": "L1Loss",
         "batch_size": 2}
NETS = ("netG_A", "netG_B", "netD_A", "netD_B")
SALTS = {"netG_A": 0, "netG_B": 300, "netD_A": 100, "netD_B": 400}
LOSS_KEYS = ("G", "G_A", "G_B", "D_A", "D_B", "cycle_A", "cycle_B", "idt_A", "idt_B")
VARIANTS = {"bg": (1.0, 2, True), "nobg": (1.0, 2, False), "idt05": (0.5, 0, True)}        # lambda_idt, pool_size, background in the batch
STEPS, TORCH_SEED = 4, 0
POOL_SIZE, POOL_QUERIES, POOL_BATCH = 3, 40, 3


def model_config(lambda_idt, pool_size):
    return {"name": "CycleGAN", "netG_A_config": {"name": "resnetGenerator9"}, "netG_B_config": {"name": "resnetGenerator9"},
            "netD_A_config": {"name": "patchGAN70x70"}, "netD_B_config": {"name": "patchGAN70x70"}, "lambda_A": 10, "lambda_B": 10,
            "lambda_idt": lambda_idt, "pool_size": pool_size}


def batch(background):
    b = {"real_A": image((2, 1, 32, 32), 4), "real_B": image((2, 1, 32, 32), 5).flip(-1)}
    if background:
        b["background"] = image((2, 1, 32, 32), 7).flip(-2)
    return b


def checksums(model):
    out = []
    for name in NETS:
        ps = [p.detach().double() for p in getattr(model, name).parameters()]
        out.append([float(sum(p.sum() for p in ps)), float(sum(p.abs().sum() for p in ps))])
    return np.array(out)


def grad_norms(model):
    return np.array([float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in getattr(model, n).parameters() if p.grad is not None)))
                     for n in NETS])


def run(model, background, scaler=None, device="cpu"):
    """STEPS consecutive steps -> (losses [STEPS, 9], gradient norms [STEPS, 4], parameter checksums [4, 2], stream positions [2])."""
    ident = {"prediction": lambda t: t, "label": lambda t: t}
    losses, norms = [], []
    for _ in range(STEPS):
        b = {k: v.to(device) for k, v in batch(background).items()}
        _, l = model.perform_training_step(b, scaler, ident, device)
        losses.append([float(l[k]) for k in LOSS_KEYS])
        norms.append(grad_norms(model))
    return np.array(losses), np.array(norms), checksums(model), np.array([random.random(), float(torch.rand(1))])


def pool_batches():
    """The 40 batches of the pool fixture: constant 2 x 2 planes carrying serial numbers 1, 2, 3, ..."""
    serial = torch.arange(1, POOL_QUERIES * POOL_BATCH + 1, dtype=torch.float32).reshape(POOL_QUERIES, POOL_BATCH, 1, 1, 1)
    return serial.expand(POOL_QUERIES, POOL_BATCH, 1, 2, 2).contiguous()


def run_pool(pool):
    """-> (returned serial numbers [40, 3], stream position)."""
    got = [pool.query(b)[:, 0, 0, 0].clone() for b in pool_batches()]
    return torch.stack(got).numpy().astype(np.int64), random.random()


def _count_exchanges(pool):
    """Wrap a reference pool's query: counts the calls after which a stored image is another object than before."""
    inner, counter = pool.query, [0]

    def query(images):
        before = [id(t) for t in getattr(pool, "images", [])]
        out = inner(images)
        after = [id(t) for t in getattr(pool, "images", [])]
        counter[0] += int(len(before) == len(after) and before != after)
        return out
    pool.query = query
    return counter


def main():
    warnings.filterwarnings("ignore")
    torch.set_num_threads(min(torch.get_num_threads(), 8))
    sys.path.insert(0, "/root/reference")
    monai = MagicMock()
    monai.data.decollate_batch = lambda t: [t[i] for i in range(t.shape[0])]
    for m in ["monai", "monai.data", "monai.losses", "monai.networks", "monai.networks.nets", "monai.networks.blocks", "monai.networks.layers",
              "monai.metrics", "monai.transforms", "monai.utils", "monai.config", "skimage", "skimage.filters", "skimage.morphology", "nibabel",
              "prettytable", "natsort", "torchvision", "torchvision.models", "torchvision.transforms", "torchvision.transforms.functional", "matplotlib",
              "matplotlib.pyplot", "rich", "rich.progress", "rich.live", "rich.spinner", "rich.console", "models.oof", "models.frangi", "models.skrgan",
              "models.nice_gan", "models.cut", "models.negcut", "models.dclgan", "models.noise_model", "utils.cldice"]:
        sys.modules.setdefault(m, monai if m == "monai" else MagicMock())
    sys.modules["monai.data"] = monai.data
    import importlib
    ref_nets = importlib.import_module("models.networks")
    ref_cg = importlib.import_module("models.cycle_gan")
    from torch.amp import GradScaler
    from utils.enums import Phase
    MODEL_DICT = {"resnetGenerator9": ref_nets.resnetGenerator9, "patchGAN70x70": ref_nets.patchGAN70x70}
    out = {}
    for tag, (lambda_idt, pool_size, background) in VARIANTS.items():
        for seed in range(64):
            torch.manual_seed(TORCH_SEED)
            cfg = model_config(lambda_idt, pool_size)
            cfg.pop("name")
            model = ref_cg.CycleGAN(phase=Phase.TRAIN, MODEL_DICT=MODEL_DICT, inference=None, **cfg)
            config = {"General": {"device": "cpu", "amp": False}, "Train": dict(TRAIN), "Output": {"save_dir": "/tmp"}}
            model.initialize_model_and_optimizer(None, ref_nets.init_weights, config, argparse.Namespace(start_epoch=0, epoch="latest"), None, Phase.TRAIN)
            for name in NETS:
                he_weights(getattr(model, name), SALTS[name])
            model.train()
            counters = [_count_exchanges(model.fake_A_pool), _count_exchanges(model.fake_B_pool)]
            torch.manual_seed(TORCH_SEED)
            random.seed(seed)
            losses, gnorm, sums, stream = run(model, background, GradScaler("cpu", enabled=False))
            if pool_size == 0 or all(c[0] > 0 for c in counters):
                break
        else:
            raise SystemExit(f"{tag}: no random seed below 64 makes both pools exchange")
        out[f"{tag}_losses"], out[f"{tag}_grad_norms"], out[f"{tag}_param_sums"], out[f"{tag}_stream"] = losses, gnorm, sums, stream
        out[f"{tag}_random_seed"] = np.array(seed)
        print(tag, "random seed", seed, "exchanges (A, B)", [c[0] for c in counters], losses, gnorm, sums, stream, sep="\n")
    for seed in range(64):
        random.seed(seed)
        pool = ref_cg.ImagePool(POOL_SIZE)
        got, pos = run_pool(pool)
        first = np.arange(1, POOL_QUERIES * POOL_BATCH + 1).reshape(POOL_QUERIES, POOL_BATCH)[:, :1]
        # an image that comes back within its own batch went through a slot that an earlier image of the batch had just taken
        twice = int(((got >= first) & (got != first + np.arange(POOL_BATCH))).any(axis=1).sum())
        if twice > 0:
            break
    else:
        raise SystemExit("no random seed below 64 draws one slot twice in a batch")
    out["pool_returned"], out["pool_final"] = got, torch.cat(pool.images)[:, 0, 0, 0].numpy().astype(np.int64)
    out["pool_stream"], out["pool_random_seed"] = np.array(pos), np.array(seed)
    print("pool: random seed", seed, "batches with one slot drawn twice:", twice, "final", out["pool_final"])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
