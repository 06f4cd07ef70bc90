"""GPU time of the sketch-filter baseline (csrc/morph.hip) per image at 304^2 and 1216^2, batches of 1 and 8: the area opening of
the filter's Gaussian plane, the area closing of its opened plane, and the whole filter, on an image of the OOF fixtures (octa,
full) and on a constant image -- the opening's worst case: every pixel is a seed and grows a full region; the filter itself is
NaN there and skips its floods, so only the opening and the closing are timed on it. HIP events around `reps` calls after a
warm-up, three times (median, minimum and maximum are printed with reps). The same work on one CPU core in the same run: scipy.ndimage
and the union-find stand-in for scikit-image (tools/skr_scipy.py, pure Python -- scikit-image's own Cython max-tree is not on
hand and would be far faster), once. Output: stdout."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy import ndimage as ndi  # noqa: E402

import skr_scipy  # noqa: E402
from octa_autosegmentation_amd.models import skrgan  # noqa: E402
from test_oof import CASES  # noqa: E402


def gpu_ms(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    reps = int(min(200, max(3, 0.3 / max(time.perf_counter() - t, 1e-6))))
    runs = []
    for _ in range(3):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        t1.synchronize()
        runs.append(t0.elapsed_time(t1) / reps)
    return sorted(runs)[1], min(runs), max(runs), reps


def cpu_filter(img):
    """the reference's chain on the stand-in; (seconds of the opening, of the closing, of the whole filter)"""
    t0 = time.perf_counter()
    m = np.sqrt(ndi.sobel(img, 0) ** 2 + ndi.sobel(img, 1) ** 2)
    m -= m.min()
    m /= m.max()
    g = ndi.gaussian_filter(m, sigma=2)
    t1 = time.perf_counter()
    o = skr_scipy.area_opening(g, 64)
    t2 = time.perf_counter()
    o -= o.min()
    o /= o.max()
    t3 = time.perf_counter()
    c = skr_scipy.area_closing(o, 64)
    t4 = time.perf_counter()
    c -= c.min()
    c /= c.max()
    return t2 - t1, t4 - t3, time.perf_counter() - t0


def main():
    torch.cuda.set_device(0)
    torch.set_num_threads(1)
    print(f"device: {torch.cuda.get_device_name(0)}")
    print(f"{'image':>14} {'B':>3} {'what':>8} {'ms/image':>10} {'(min .. max of 3)':>22} {'reps':>5} {'CPU s/image':>12}")
    for name, n in (("octa", 304), ("full", 1216)):
        img = CASES[name]["img"]
        assert img.shape == (n, n)
        cpu = dict(zip(("opening", "closing", "filter"), cpu_filter(img)))
        t = time.perf_counter()
        skr_scipy.area_opening(np.full((n, n), np.float32(0.5)), 64)
        cpu_const = time.perf_counter() - t
        for b in (1, 8):
            x = torch.from_numpy(img).cuda()[None, None].repeat(b, 1, 1, 1).contiguous()
            _, filt, opened, _ = skrgan.sketch_stages(x)
            const = torch.full_like(x, 0.5)
            rows = [(f"{name} {n}^2", "opening", lambda: skrgan.area_opening(filt), cpu["opening"]),
                    (f"{name} {n}^2", "closing", lambda: skrgan.area_closing(opened), cpu["closing"]),
                    (f"{name} {n}^2", "filter", lambda: skrgan.sketch_filter(x), cpu["filter"]),
                    (f"const {n}^2", "opening", lambda: skrgan.area_opening(const), cpu_const),
                    (f"const {n}^2", "closing", lambda: skrgan.area_closing(const), cpu_const)]
            for label, what, fn, cpu_s in rows:
                ms, lo, hi, reps = gpu_ms(fn)
                print(f"{label:>14} {b:>3} {what:>8} {ms / b:>10.4f} {f'{lo / b:.4f} .. {hi / b:.4f}':>22} {reps:>5} {cpu_s:>12.2f}", flush=True)


if __name__ == "__main__":
    main()
