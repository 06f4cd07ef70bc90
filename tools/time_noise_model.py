"""tools/time_noise_model.py -- per-sample cost of the paper's noise model at the training configs' image size (304x304), in ONE run:
  * the device path (control-point draws on the host, upload, csrc/noise_model.hip) at B = 1 and B = 4, wall clock to a device synchronise;
  * the kernel alone (device events around back-to-back launches on resident inputs) and its share of the device-path time;
  * the host restatement (data/noise_model.py, torch on the CPU) on ONE thread, what a CPU tensor costs and what the reference's own class costs;
  * NoiseModeld end to end as the loader calls it, per sample;
  * the kernel's backward (octa_noise_model_backward: pixel pass + gather) at B = 1 and B = 4, launch to launch;
  * the training step of configs/config_ves_seg-S_AA.yml at B = 4 (304^2 image and background, 1216^2 label: the three-step ascent loop of
    models/noise_model_at.py, then the ordinary step) beside the plain step of configs/config_ves_seg-S.yml on the same box.
Needs a GPU.   python tools/time_noise_model.py [--reps 200] [--host-reps 20]"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from octa_autosegmentation_amd.data import data_transforms as T  # noqa: E402
from octa_autosegmentation_amd.data import gpu_augment, noise_model  # noqa: E402

N = 304
LAMBDAS = (1, 0.7, 0.3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_noise_model.py measures on the GPU; none is visible")
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    print(f"noise model per {N}x{N} sample (ms), {a.reps} repetitions after 5 warm-up rounds, on {torch.cuda.get_device_name(dev)}")
    for B in (1, 4):
        img, bg = torch.rand(B, N, N).to(dev), torch.rand(B, N, N).to(dev)
        draws = noise_model.NoiseModelDraws((9, 9))

        def path():
            grids = torch.cat(draws.control_points(B), dim=1)
            seed = int(torch.empty((), dtype=torch.int64).random_().item())
            return gpu_augment.noise_model(img, bg, grids, seed, *LAMBDAS)

        for i in range(a.reps + 5):
            if i == 5:
                torch.cuda.synchronize(); t0 = time.perf_counter()
            path()
        torch.cuda.synchronize()
        whole = 1e3 * (time.perf_counter() - t0) / a.reps

        grids = torch.cat(draws.control_points(B), dim=1).to(dev)
        for _ in range(5):
            gpu_augment.noise_model(img, bg, grids, 1, *LAMBDAS)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.reps):
            gpu_augment.noise_model(img, bg, grids, i, *LAMBDAS)
        e1.record()
        torch.cuda.synchronize()
        kern = e0.elapsed_time(e1) / a.reps
        print(f"  device path B={B}: {whole / B:8.4f} per sample ({whole:8.4f} per call: draws + upload + kernel); kernel alone, launch to launch "
              f"{kern / B:8.4f} per sample ({kern:8.4f} per call) = {100 * kern / whole:5.1f} % of the call")

    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    img, bg = torch.rand(1, 1, N, N), torch.rand(1, 1, N, N)
    draws = noise_model.NoiseModelDraws((9, 9))
    for i in range(a.host_reps + 2):
        if i == 2:
            t0 = time.perf_counter()
        noise_model.noise_model_host(img, bg, draws.control_points(1), *LAMBDAS)
    print(f"  host restatement, 1 thread: {1e3 * (time.perf_counter() - t0) / a.host_reps:8.3f} per sample")
    torch.set_num_threads(threads)

    t = T.NoiseModeld(["image"])
    sample = {"image": torch.rand(1, N, N).to(dev), "background": torch.rand(1, N, N).to(dev)}
    for i in range(a.reps + 5):
        if i == 5:
            torch.cuda.synchronize(); t0 = time.perf_counter()
        t(sample)
    torch.cuda.synchronize()
    print(f"  NoiseModeld end to end (CUDA sample [1, {N}, {N}]): {1e3 * (time.perf_counter() - t0) / a.reps:8.4f} per sample")

    for B in (1, 4):
        img, bg, dout = (torch.rand(B, N, N).to(dev) for _ in range(3))
        grids = torch.cat(noise_model.NoiseModelDraws((9, 9)).control_points(B), dim=1).to(dev)
        for _ in range(5):
            gpu_augment.noise_model_backward(dout, img, bg, grids, 1, *LAMBDAS)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.reps):
            gpu_augment.noise_model_backward(dout, img, bg, grids, i, *LAMBDAS)
        e1.record()
        torch.cuda.synchronize()
        kern = e0.elapsed_time(e1) / a.reps
        print(f"  backward B={B}: launch to launch {kern / B:8.4f} per sample ({kern:8.4f} per call, both kernels and the scratch allocation)")

    import yaml
    from octa_autosegmentation_amd.models.segmentation_trainer import SegmentationTrainer
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    B, steps = 4, max(10, a.reps // 10)
    x, bg = torch.rand(B, 1, N, N).to(dev), (torch.rand(B, 1, N, N) * 0.6).to(dev)
    y = (torch.nn.functional.interpolate(x, size=(4 * N, 4 * N), mode="bilinear") > 0.6).float()
    x_big = torch.nn.functional.interpolate(x, size=(4 * N, 4 * N), mode="bilinear")
    # dtypes as the loader delivers them under General.amp: image and label in bf16 (CastToTyped), the background in float32
    h = lambda t: t.to(torch.bfloat16)
    for name, batch in (("config_ves_seg-S_AA.yml", {"image": h(x), "background": bg, "label": h(y)}), ("config_ves_seg-S.yml", {"image": h(x_big), "label": h(y)})):
        tr = SegmentationTrainer(yaml.safe_load(open(os.path.join(root, "configs", name))), dev)
        for i in range(steps + 3):
            if i == 3:
                torch.cuda.synchronize(); t0 = time.perf_counter()
            tr.perform_training_step(dict(batch))
        torch.cuda.synchronize()
        print(f"  training step of {name} at B={B} ({N}^2 -> {4 * N}^2): {1e3 * (time.perf_counter() - t0) / steps:8.3f} ms per step ({steps} steps)")


if __name__ == "__main__":
    main()
