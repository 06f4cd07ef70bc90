"""GPU time of the OOF baseline (csrc/oof.hip) per image at 304^2, 400^2 and 1216^2, batches of 1 and 8: HIP events around
`reps` calls after a warm-up, with the bytes the kernels move per image (a model computed from the shape) and the rate that
gives. Output: profiles/oof_timing.log."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from octa_autosegmentation_amd.models.oof import OOF  # noqa: E402


def bytes_per_image(h, w):
    """HBM bytes the launches of one image read and write: complex-double planes of 16 h w bytes, real planes of 8 h w."""
    c, r = 16 * h * w, 8 * h * w
    fwd = (4 * h * w + c) + 2 * c                       # rows: float32 in, transposed complex out; columns: in and out
    per_pair = c + 3 * c + 3 * 4 * c                    # spectrum: F in, 3 planes out; inverse FFT: 2 passes x (in + out) x 3 planes
    single = c + 2 * c + 2 * 4 * c
    eig = 2 * c + r + r                                 # A and C in, running output in and out
    norm = r + 2 * r                                    # max, then in and out
    return fwd + 2 * per_pair + single + 5 * eig + norm


def main():
    torch.cuda.set_device(0)
    f = OOF()
    g = torch.Generator(device="cuda").manual_seed(0)
    print(f"device: {torch.cuda.get_device_name(0)}")
    print(f"{'size':>10} {'B':>3} {'ms/image':>10} {'ms/call':>10} {'MB/image':>10} {'GB/s':>8}")
    for n in (304, 400, 1216):
        for b in (1, 8):
            x = torch.rand(b, 1, n, n, device="cuda", generator=g)
            for _ in range(3):
                f(x)
            torch.cuda.synchronize()
            reps = max(3, int(200 / (b * (n / 304) ** 2)))
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                f(x)
            t1.record()
            t1.synchronize()
            ms = t0.elapsed_time(t1) / reps
            mb = bytes_per_image(n, n) / 1e6
            print(f"{n}x{n:<5} {b:>3} {ms / b:>10.3f} {ms:>10.3f} {mb:>10.1f} {mb * b / ms:>8.1f}", flush=True)


if __name__ == "__main__":
    main()
