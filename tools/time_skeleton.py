"""GPU time of the clDice skeleton (csrc/skeleton.hip) on the 1216^2 pair of tests/test_skeleton_gpu.py: the rasteriser
fixture's label and a perturbed copy (dilated, 5 % of the pixels dropped).

  * octa_skeletonize at B = 2 (and each image alone): ms per call, the double passes and launches it took;
  * the whole ClDiceMetric call, and MetricsManager(VALIDATION) per sample with and without the clDice column;
  * the same pair through skeletonize_host on this box;
  * --validate: validate.py on configs/config_ves_seg-S.yml, seconds per sample with the clDice column and with the column taken
    out (the parent's metric set), alternating in one process. The checkpoint holds freshly initialised weights and the samples are
    synthetic, so the predictions are not vessel trees: the double passes they took are printed beside the times.

Host clock around work that ends in a device synchronise; every shape is warmed up first."""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from octa_autosegmentation_amd.utils import metrics as metrics_mod  # noqa: E402
from octa_autosegmentation_amd.utils import skeleton  # noqa: E402
from octa_autosegmentation_amd.utils.enums import Phase  # noqa: E402

CHUNK = 8           # SKEL_CHUNK of csrc/skeleton.hip


def timed(f, n):
    f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def pair():
    from scipy.ndimage import binary_dilation
    g = np.load(os.path.join(ROOT, "tests", "golden", "raster_golden.npz"))
    label = np.unpackbits(np.asarray(g["graph0_label_packed"])).reshape(1216, 1216).astype(np.uint8)
    pred = (binary_dilation(label) & (np.random.default_rng(0).random(label.shape) >= 0.05)).astype(np.uint8)
    return label, pred


def launches(passes):
    """pack + 2 per double pass of every chunk the host loop ran + unpack (+ one memset and one flag copy per chunk)."""
    chunks = -(-passes // CHUNK)
    return 2 + 2 * CHUNK * chunks, chunks


def kernel_and_metric(n):
    label, pred = pair()
    dl, dp = torch.from_numpy(label).cuda(), torch.from_numpy(pred).cuda()
    both = torch.stack([dl, dp])
    for name, m in (("label alone", dl), ("perturbed alone", dp), ("pair, B = 2", both)):
        out, passes = skeleton.skeletonize_device(m, return_passes=True)
        k, chunks = launches(passes)
        ms = timed(lambda: skeleton.skeletonize_device(m), n)
        print(f"octa_skeletonize {name}: {ms:.3f} ms per call ({passes} double passes, {k} kernel launches, {chunks} flag reads; "
              f"{int(out.sum())} skeleton pixels; includes the wrapper's != 0 and uint8 copy)", flush=True)
    y_pred, y = [dp[None].float()], [dl[None]]
    cl = metrics_mod.ClDiceMetric()
    print(f"ClDiceMetric, one sample: {timed(lambda: cl(y_pred, y), n):.3f} ms per call; score {float(cl.scores[0]):.6f}", flush=True)
    full = metrics_mod.MetricsManager(Phase.VALIDATION)
    without = metrics_mod.MetricsManager(Phase.VALIDATION)
    del without.metrics["ClDice"]
    a = b = 0.0
    for _ in range(3):                                   # alternate the two sets
        a += timed(lambda: full(y_pred, y), max(1, n // 3)) / 3
        b += timed(lambda: without(y_pred, y), max(1, n // 3)) / 3
    print(f"MetricsManager(VALIDATION), one sample: {a:.3f} ms with clDice, {b:.3f} ms without (the parent's set)", flush=True)
    t0 = time.perf_counter()
    hl, hp = skeleton.skeletonize_host(label), skeleton.skeletonize_host(pred)
    print(f"skeletonize_host, the same pair: {(time.perf_counter() - t0) * 1e3:.0f} ms (numpy, one thread)", flush=True)
    got = skeleton.skeletonize_device(both).cpu().numpy()
    assert np.array_equal(got[0], hl) and np.array_equal(got[1], hp)
    print("device skeletons equal the host's", flush=True)


def validate_ab(samples, reps, device="cuda:0"):
    import yaml
    from PIL import Image
    import validate as validate_cli
    from octa_autosegmentation_amd.models.model import define_model
    from octa_autosegmentation_amd.utils.checkpoints import save_model
    label, _ = pair()
    cfg_path = os.path.join(ROOT, "configs", "config_ves_seg-S.yml")
    with open(cfg_path) as f:
        config = yaml.safe_load(f)
    config["General"]["device"] = device
    with tempfile.TemporaryDirectory() as tmp:
        for sub in ("images", "labels"):
            os.makedirs(os.path.join(tmp, sub))
        rng = np.random.default_rng(1)
        for i in range(samples):
            lab = np.rot90(label, i % 4) if i < 4 else np.flipud(np.rot90(label, i % 4))
            img = lab.reshape(304, 4, 304, 4).mean(axis=(1, 3)) * 200 + rng.integers(0, 56, (304, 304))
            Image.fromarray(img.astype(np.uint8)).save(os.path.join(tmp, "images", f"{i}.png"))
            Image.fromarray((lab * 255).astype(np.uint8)).save(os.path.join(tmp, "labels", f"{i}.png"))
        torch.manual_seed(0)
        model = define_model(config, phase=Phase.VALIDATION)
        save_model(os.path.join(tmp, "run"), model.model, None, 1, config, "best_model")
        dump = lambda p: yaml.safe_dump({"files": p}, default_flow_style=True).strip()
        argv = ["--config_file", cfg_path, "--num_workers", "0", "--Validation.data.image", dump(os.path.join(tmp, "images", "*.png")),
                "--Validation.data.label", dump(os.path.join(tmp, "labels", "*.png")), "--Output.save_dir", os.path.join(tmp, "run"), "--General.device", device]

        passes = []
        device_fn = skeleton.skeletonize_device

        def logging_device(mask, return_passes=False):
            out, p = device_fn(mask, return_passes=True)
            passes.append(p)
            return (out, p) if return_passes else out

        class Parent(metrics_mod.MetricsManager):
            def __init__(self, phase=Phase.TRAIN):
                super().__init__(phase)
                self.metrics.pop("ClDice", None)

        def run(with_cldice):
            saved = metrics_mod.MetricsManager
            metrics_mod.MetricsManager = saved if with_cldice else Parent
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = validate_cli.main(argv)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / samples, res
            finally:
                metrics_mod.MetricsManager = saved

        run(True)                                            # warm-up: code objects, the loader's caches
        skeleton.skeletonize_device = logging_device
        _, res = run(True)
        skeleton.skeletonize_device = device_fn
        print(f"validate.py on the S config, {samples} samples (initial weights): {res}")
        print(f"double passes of the samples' (prediction, label) pairs: {passes}")
        a, b = [], []
        for _ in range(reps):
            a.append(run(True)[0])
            b.append(run(False)[0])
        print(f"validate.py seconds per sample: with clDice {np.mean(a):.4f} (min {min(a):.4f}, max {max(a):.4f}), "
              f"without (the parent's metric set) {np.mean(b):.4f} (min {min(b):.4f}, max {max(b):.4f}); {reps} alternating runs each", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--validate", action="store_true")
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    torch.cuda.set_device(0)
    print(torch.cuda.get_device_name(0), flush=True)
    kernel_and_metric(args.calls)
    if args.validate:
        validate_ab(args.samples, args.reps)


if __name__ == "__main__":
    main()
