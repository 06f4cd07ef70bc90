"""tools/time_augment_crop.py -- the Giarratano set-up's augmentation of one mini-batch on the GPU, two ways, in one process:
  (a) resize_bilinear + flip_rot90_rotate over the full 1216^2 frame, then the 360^2 slice made contiguous, for image and label;
  (b) resize_bilinear + flip_rot90_rotate_window, which computes the 360^2 window only (csrc/augment.hip).
Inputs as in training: B = 4, a 304^2 uint8 image and a 1216^2 uint8 label per sample, window 360 x 360 at seeded offsets, seeded flips, turns and
angles. Both ways give the same tensors (checked before timing). Device events around each call, the two ways alternating, after a warm-up;
the figure is the median over --reps calls, with the quartiles as the spread. Needs a GPU.   python tools/time_augment_crop.py [--reps 200]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from octa_autosegmentation_amd.data import gpu_augment as A  # noqa: E402

B, SMALL, N, WIN = 4, 304, 1216, 360


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_augment_crop.py measures on the GPU; none is visible")
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.RandomState(0)
    image = torch.from_numpy(rng.randint(0, 256, (B, SMALL, SMALL)).astype(np.uint8)).to(dev)
    label = torch.from_numpy(((rng.rand(B, N, N) < 0.2) * 255).astype(np.uint8)).to(dev)
    ang = torch.from_numpy(rng.uniform(-0.1745, 0.1745, B).astype(np.float32)).to(dev)
    k = torch.from_numpy(rng.randint(0, 4, B).astype(np.int32)).to(dev)
    f = torch.from_numpy(rng.randint(0, 2, B).astype(np.int32)).to(dev)
    oy_h, ox_h = rng.randint(0, N - WIN + 1, B), rng.randint(0, N - WIN + 1, B)
    oy, ox = (torch.from_numpy(o.astype(np.int32)).to(dev) for o in (oy_h, ox_h))
    mul = torch.full((B,), 1.0 / 255.0, device=dev)
    add = torch.zeros(B, device=dev)
    pairs = ((image, None), (label, 0.1))

    def full_then_slice():
        out = []
        for x, thr in pairs:
            y = A.flip_rot90_rotate(A.resize_bilinear(x, (N, N), mul, add), ang, k, f, thr)
            out.append(torch.stack([y[b, oy_h[b]:oy_h[b] + WIN, ox_h[b]:ox_h[b] + WIN] for b in range(B)]).contiguous())
        return out

    def window():
        return [A.flip_rot90_rotate_window(A.resize_bilinear(x, (N, N), mul, add), ang, k, f, thr, (WIN, WIN), oy, ox) for x, thr in pairs]

    for u, v in zip(full_then_slice(), window()):
        assert u.shape == v.shape == (B, WIN, WIN) and torch.equal(u, v), "the two ways disagree"
    ways = (("(a) full frame + slice", full_then_slice), ("(b) window kernel", window))
    ms = {name: [] for name, _ in ways}
    for i in range(a.warmup + a.reps):
        for name, fn in ways:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))
    print(f"{torch.cuda.get_device_name(dev)}: B = {B}, image {SMALL}^2 + label {N}^2 uint8 -> {WIN}^2 windows of the {N}^2 frame, both tensors; "
          f"ms per mini-batch, median [quartiles] of {a.reps} calls after {a.warmup} warm-up calls, the two ways alternating")
    for name, _ in ways:
        q1, med, q3 = np.percentile(ms[name], [25, 50, 75])
        print(f"  {name:26s} {med:8.3f}  [{q1:.3f}, {q3:.3f}]")
    # what the rotate step alone has to move per tensor and sample (float32): the write of the frame or of the window
    print(f"  rotate output per tensor and sample: {N * N * 4 / 1e6:.2f} MB (a)  {WIN * WIN * 4 / 1e6:.2f} MB (b)")


if __name__ == "__main__":
    main()
