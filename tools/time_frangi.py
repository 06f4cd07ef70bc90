"""GPU time of the Frangi baseline (csrc/frangi.hip) per image at 304^2 and 1216^2, batches of 1 and 8: HIP events around `reps`
calls after a warm-up of every shape, repeated three times (the spread is printed), with the bytes the launches move per image
(a model computed from the shape) and the rate that gives. A call includes the workspace allocation from torch's caching
allocator and 18 launches. Output: profiles/frangi_timing.log."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from octa_autosegmentation_amd.models.frangi import Frangi  # noqa: E402

SCALES = 2      # distinct scales of the reference's (0.5, 2, 0.5)


def bytes_per_image(h, w):
    """HBM bytes the launches of one image read and write, float32 planes of 4 h w bytes (tile halos come from the caches):
    per scale 2 two-output passes (1 in, 2 out) and 6 one-output passes (1 in, 1 out); the maximum of s reads 3 planes; the
    vesselness reads 3 planes per scale and writes one float64 plane."""
    p = 4 * h * w
    return SCALES * (2 * 3 * p + 6 * 2 * p) + 3 * p + (3 * SCALES * p + 2 * p)


def main():
    torch.cuda.set_device(0)
    f = Frangi()
    g = torch.Generator(device="cuda").manual_seed(0)
    print(f"device: {torch.cuda.get_device_name(0)}")
    print(f"{'size':>10} {'B':>3} {'ms/image':>10} {'(min .. max of 3)':>20} {'ms/call':>10} {'MB/image':>10} {'GB/s':>8}")
    for n in (304, 1216):
        for b in (1, 8):
            x = torch.rand(b, 1, n, n, device="cuda", generator=g)
            for _ in range(5):
                f(x)
            torch.cuda.synchronize()
            reps = max(20, int(4000 / (b * (n / 304) ** 2)))
            runs = []
            for _ in range(3):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(reps):
                    f(x)
                t1.record()
                t1.synchronize()
                runs.append(t0.elapsed_time(t1) / reps)
            ms = sorted(runs)[1]
            mb = bytes_per_image(n, n) / 1e6
            print(f"{n}x{n:<5} {b:>3} {ms / b:>10.4f} {f'{min(runs) / b:.4f} .. {max(runs) / b:.4f}':>20} {ms:>10.4f} {mb:>10.1f} {mb * b / ms:>8.1f}", flush=True)


if __name__ == "__main__":
    main()
