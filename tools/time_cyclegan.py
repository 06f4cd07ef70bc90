"""tools/time_cyclegan.py -- the CycleGAN step (models/cycle_gan.py) on one GPU at the shape of configs/config_cycle_gan.yml: B = 4,
304 x 304, bf16 autocast, lambda_idt 1, pool_size 50. Prints, from one run:

  * ms per step with the fused elementwise tail (csrc/gan_loss.hip) and with `gan_loss.USE_FUSED_GAN_LOSS = False` (the torch
    composition), alternating windows of the two in one process, median of the windows;
  * device kernel launches per step of both (torch.profiler's device activities of one step; "not measured" if the profiler gives none);
  * the GAN-seg step (models/gan_seg_model.py, B = 4, 304 x 304 -> 1216 x 1216) in the same run, for scale.

Usage: python tools/time_cyclegan.py [--steps 20] [--windows 3]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("OCTA_STRICT", "1")          # the measured path is the HIP path or nothing

B, N = 4, 304


def cycle_gan():
    from argparse import Namespace
    from copy import deepcopy
    from octa_autosegmentation_amd.models import networks
    from octa_autosegmentation_amd.models.model import define_model
    from octa_autosegmentation_amd.utils.enums import Phase
    net = lambda n: {"name": n}
    config = {"General": {"device": "cuda:0", "amp": True,
                          "model": {"name": "CycleGAN", "netG_A_config": net("resnetGenerator9"), "netG_B_config": net("resnetGenerator9"),
                                    "netD_A_config": net("patchGAN70x70"), "netD_B_config": net("patchGAN70x70"), "lambda_A": 10, "lambda_B": 10,
                                    "lambda_idt": 1, "pool_size": 50}},
              "Train": {"lr": 2e-4, "epochs": 100, "epochs_decay": 0, "loss_criterionGAN": "LSGANLoss", "loss_criterionCycle": "L1Loss",
                        "loss_criterionIdt": "L1Loss"}, "Output": {"save_dir": "."}}
    model = define_model(deepcopy(config), Phase.TRAIN)
    model.initialize_model_and_optimizer(None, networks.init_weights, config, Namespace(start_epoch=0, epoch="latest"), None, Phase.TRAIN)
    model.train()
    g = torch.Generator(device="cuda").manual_seed(0)
    batch = {k: torch.rand(B, 1, N, N, device="cuda", generator=g).to(torch.bfloat16) for k in ("real_A", "real_B", "background")}
    return lambda: model.perform_training_step(batch, None, None, torch.device("cuda:0"))


def gan_seg():
    from octa_autosegmentation_amd.models.gan_seg_trainer import GanSegTrainer
    cfg = {"General": {"amp": True, "model": {"name": "GanSegModel", "model_g": {"name": "resnetGenerator9"}, "model_d": {"name": "patchGAN70x70"},
                                              "model_s": {"name": "DynUNet", "spatial_dims": 2, "in_channels": 1, "out_channels": 1,
                                                          "kernel_size": [3, 3, 3, 3, 3], "strides": [1, 2, 2, 2, 1], "upsample_kernel_size": [1, 2, 2, 2, 1]},
                                              "compute_identity": False, "compute_identity_seg": True}},
           "Train": {"lr": 2e-4, "loss_dg": "LSGANLoss", "loss_s": "DiceBCELoss"}}
    tr = GanSegTrainer(cfg, "cuda:0")
    g = torch.Generator(device="cuda").manual_seed(1)
    batch = {"real_A": torch.rand(B, 1, N, N, device="cuda", generator=g), "real_B": torch.rand(B, 1, N, N, device="cuda", generator=g),
             "real_A_seg": (torch.rand(B, 1, 4 * N, 4 * N, device="cuda", generator=g) > 0.8).float()}
    return lambda: tr.perform_training_step(batch)


def window(step, steps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / steps


def launches(step):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n if n > 0 else "not measured"
    except Exception as exc:          # a profiler that does not run is not a reason to lose the timings
        print(f"launch count not measured: {exc}", file=sys.stderr)
        return "not measured"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    from octa_autosegmentation_amd.models import gan_loss
    torch.manual_seed(0)
    random.seed(0)
    step = cycle_gan()

    def with_tail(fused, f):
        old, gan_loss.USE_FUSED_GAN_LOSS = gan_loss.USE_FUSED_GAN_LOSS, fused
        try:
            return f()
        finally:
            gan_loss.USE_FUSED_GAN_LOSS = old

    for fused in (True, False):                      # warm both forms: code objects, weight packs, the pools' first fill
        with_tail(fused, lambda: window(step, 5))
    times = {True: [], False: []}
    for _ in range(args.windows):
        for fused in (True, False):
            times[fused].append(with_tail(fused, lambda: window(step, args.steps)))
    counts = {fused: with_tail(fused, lambda: launches(step)) for fused in (True, False)}
    seg = gan_seg()
    window(seg, 5)
    seg_ms = [window(seg, args.steps) for _ in range(args.windows)]
    out = {"gpu": torch.cuda.get_device_name(0), "batch": B, "size": N, "steps_per_window": args.steps, "windows": args.windows,
           "cyclegan_fused_ms": round(statistics.median(times[True]), 3), "cyclegan_composed_ms": round(statistics.median(times[False]), 3),
           "cyclegan_fused_ms_windows": [round(t, 3) for t in times[True]], "cyclegan_composed_ms_windows": [round(t, 3) for t in times[False]],
           "cyclegan_fused_launches": counts[True], "cyclegan_composed_launches": counts[False],
           "ganseg_ms": round(statistics.median(seg_ms), 3), "runs": 1}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
