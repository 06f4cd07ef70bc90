"""GPU: the Menten et al. augmentation through the kernels of csrc/menten.hip, against the reference's own outputs
(tests/golden/menten_golden.npz). float64 images within 1e-12 absolute: values lie in [0, 1] and a float64 sum of at most 2 x 81 positive
taps adding up to 1 errs by about 2e-14, while the smallest tap of the sigma = 10 kernel is 1.3e-5 -- a wrong tap, radius or boundary
rule misses by seven orders of magnitude. Labels, motion results and the floater mask are exact."""
import os

import numpy as np
import pytest
import torch

import _menten_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


@pytest.fixture(scope="module")
def dev(hip_lib_built):
    assert os.environ.get("OCTA_STRICT") == "1"          # tests/conftest.py: a host fallback of a supported layout would raise
    return torch.device("cuda", torch.cuda.current_device())


def close(t, want):
    a = t.cpu().numpy()
    assert a.dtype == want.dtype and a.shape == want.shape
    err = float(np.abs(a - want).max())
    print("max abs error", err)
    return err <= TOL


@pytest.mark.parametrize("k", C.vessel_cases())
def test_vessel_noise_kernels_match_the_reference(dev, k):
    g = C.golden()
    out, nxt, x, keep = C.run_vessel(k, dev)
    assert out.is_cuda and close(out, g[f"vessel_{k}_out"])
    assert nxt == float(g[f"vessel_{k}_next"]) and torch.equal(x, keep)
    again = C.run_vessel(k, dev)[0]
    assert torch.equal(out, again)


def test_vessel_noise_non_integral_radius_agrees_with_the_host_path(dev):
    """r = 20.5: the ring compare runs on the correctly rounded double square root instead of squared integers."""
    from octa_autosegmentation_amd.data import data_transforms as T
    x = torch.from_numpy(C.golden()["vessel_1_in"].copy())
    res = []
    for d in (torch.device("cpu"), dev):
        np.random.seed(77)
        res.append(T.BinomialVesselNoised(["image"], r=20.5)({"image": x.to(d)})["image"].cpu())
    assert (res[0] - res[1]).abs().max().item() <= TOL


@pytest.mark.parametrize("k", C.floater_cases())
def test_floater_kernels_match_the_reference(dev, k):
    g = C.golden()
    out, nxt, x, keep = C.run_floater(k, dev)
    assert out.is_cuda and close(out, g[f"floater_{k}_out"])
    assert nxt == float(g[f"floater_{k}_next"]) and torch.equal(x, keep)
    assert torch.equal(out, C.run_floater(k, dev)[0])
    if k == 3:
        assert out.dtype == torch.float32 and torch.equal(out, keep)


def test_floater_on_a_non_square_image_raises_like_the_reference(dev):
    from octa_autosegmentation_amd.data import data_transforms as T
    g = C.golden()
    x = torch.from_numpy(g["floater_4_in"].copy()).to(dev)
    np.random.seed(int(g["floater_4_seed"]))
    with pytest.raises(ValueError, match="could not be broadcast"):
        T.AddVitreousFloater(["image"], floater_chance=1.0)({"image": x})
    assert np.random.uniform() == float(g["floater_4_next"])


@pytest.mark.parametrize("n, dilations", [(48, 1), (48, 10), (48, 30), (37, 7), (300, 29)])
def test_floater_mask_is_scipys_binary_dilation(dev, n, dilations):
    """The mask alone -- Bresenham on the device, then L1 distance <= dilations by two scans -- against the host's lines dilated by scipy,
    exactly; sizes: the fixtures', an odd one, one above the 256-thread row block; a walk that leaves the image and a pixel in a corner."""
    from scipy.ndimage import binary_dilation
    from octa_autosegmentation_amd.data import gpu_augment, menten
    np.random.seed(n + dilations)
    pts = menten.floater_draws(n, n, 1.0)[0]
    pts[-1] = (n - 1, 0)                                 # ends in a corner
    pts[1] = (-5, n + 3)                                 # and leaves the image
    want = binary_dilation(menten.floater_lines_host(pts, 1.0, n, n), iterations=dilations)
    got = gpu_augment.menten_floater_mask([pts], [dilations], n, dev)
    assert got.dtype == torch.bool and got.shape == (1, n, n)
    assert np.array_equal(got[0].cpu().numpy(), want)


@pytest.mark.parametrize("seed", C.motion_seeds())
def test_motion_kernel_matches_the_reference_exactly(dev, seed):
    g = C.golden()
    img, gt, nxt, (x, y), (kx, ky) = C.run_motion(seed, dev)
    assert img.is_cuda and gt.is_cuda
    a, b = img.cpu().numpy(), gt.cpu().numpy()
    assert a.dtype == np.float64 and b.dtype == np.float32
    assert np.array_equal(a, g[f"motion_{seed}_out"]) and np.array_equal(b, g[f"motion_{seed}_gt"])
    assert nxt == float(g[f"motion_{seed}_next"])
    assert torch.equal(x, kx) and torch.equal(y, ky) and img.data_ptr() != x.data_ptr() and gt.data_ptr() != y.data_ptr()


def test_motion_on_a_float32_image_matches_the_host_path_exactly(dev):
    """dtypes are kept: a float32 image takes the 4-byte (and, shifts permitting, 16-byte) copies and float32-rounded whiteout rows."""
    from octa_autosegmentation_amd.data import data_transforms as T
    g = C.golden()
    x, y = torch.from_numpy(g["motion_in"].astype(np.float32)), torch.from_numpy(g["motion_gt"].copy())
    for seed in C.motion_seeds():
        res = []
        for d in (torch.device("cpu"), dev):
            np.random.seed(seed)
            out = T.AddMotionArtifact("image", "label")({"image": x.to(d), "label": y.to(d)})
            res.append((out["image"].cpu(), out["label"].cpu()))
        assert res[1][0].dtype == torch.float32 and torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_menten_chain_matches_the_reference(dev):
    g = C.golden()
    img, gt, nxt = C.run_menten(dev)
    assert img.is_cuda and close(img, g["menten_out"])
    assert np.array_equal(gt.cpu().numpy(), g["menten_gt"]) and gt.dtype == torch.float32
    assert nxt == float(g["menten_next"])
    img2, gt2, _ = C.run_menten(dev)
    assert torch.equal(img, img2) and torch.equal(gt, gt2)


def test_batch_of_two_equals_two_single_calls(dev):
    from octa_autosegmentation_amd.data import gpu_augment, menten
    g = C.golden()
    rng = np.random.RandomState(5)
    # vessel noise, float32 images of an odd size
    x = torch.from_numpy(rng.rand(2, 37, 70).astype(np.float32)).to(dev)
    bern = torch.from_numpy((rng.rand(2, 37, 70) < 0.1).astype(np.uint8)).to(dev)
    q = torch.from_numpy(rng.uniform(0, 0.2, (2, 37, 70))).to(dev)
    both = gpu_augment.menten_vessel_noise(x, bern, q, 1.0, 0.5, 15)
    for b in range(2):
        assert torch.equal(both[b:b + 1], gpu_augment.menten_vessel_noise(x[b:b + 1], bern[b:b + 1], q[b:b + 1], 1.0, 0.5, 15))
    # floater: walks of different lengths and dilation counts
    img = torch.from_numpy(rng.rand(2, 48, 48)).to(dev)
    np.random.seed(3)
    walks = [menten.floater_draws(48, 48, 1.0) for _ in range(2)]
    pts, dil = [w[0] for w in walks], [w[2] for w in walks]
    assert len(pts[0]) != len(pts[1]) or dil[0] != dil[1]
    both = gpu_augment.menten_floater(img, pts, dil)
    masks = gpu_augment.menten_floater_mask(pts, dil, 48, dev)
    for b in range(2):
        assert torch.equal(both[b:b + 1], gpu_augment.menten_floater(img[b:b + 1], pts[b:b + 1], dil[b:b + 1]))
        assert torch.equal(masks[b:b + 1], gpu_augment.menten_floater_mask(pts[b:b + 1], dil[b:b + 1], 48, dev))
    # motion: two different label tables (16-byte copies: every shift is a multiple of four floats)
    lab = torch.from_numpy(np.concatenate([g["motion_gt"], g["motion_gt"][:, ::-1].copy()])).to(dev)
    tables = []
    for seed in (603, 609):
        np.random.seed(seed)
        tables.append(menten.fold_cuts(48, 48, menten.motion_draws(48, 48, {'shear': 0.3, 'stretch': 0.3, 'buckle': 0.3, 'whiteout': 0.1}), 4)[0])
    both = gpu_augment.menten_motion(lab, np.stack(tables))
    for b in range(2):
        assert torch.equal(both[b:b + 1], gpu_augment.menten_motion(lab[b:b + 1], tables[b]))
    assert not torch.equal(both, lab)


def test_unsupported_layout_reports_the_host_path(dev, monkeypatch):
    """A CUDA tensor outside the kernels' layouts ([H, W] without a channel axis) raises under OCTA_STRICT=1 and warns once otherwise."""
    from octa_autosegmentation_amd.data import data_transforms as T
    x = torch.from_numpy(C.golden()["vessel_0_in"][0].copy()).to(dev)
    t = T.BinomialVesselNoised(["image"], r=20)
    with pytest.raises(T.HostFallbackError):
        t({"image": x})
    monkeypatch.setenv("OCTA_STRICT", "0")
    T._HOST_FALLBACK_WARNED.clear()
    np.random.seed(int(C.golden()["vessel_0_seed"]))
    with pytest.warns(RuntimeWarning, match="host restatement"):
        out = t({"image": x})["image"]
    assert out.is_cuda and np.array_equal(out.cpu().numpy(), C.golden()["vessel_0_out"][0])
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        t({"image": x})                                  # once


def test_loader_with_the_menten_config(dev, tmp_path, raster_golden):
    """configs/config_ves_seg-S_Menten_aug.yml's training chain over two short graphs: the loader's mini-batch has the network's shapes and
    dtype, and up to and including MentenAugmentationd the device path equals the host path for the same seeds."""
    import random
    import yaml
    from PIL import Image
    from octa_autosegmentation_amd import graph_io
    from octa_autosegmentation_amd.data import data_transforms as T
    from octa_autosegmentation_amd.data.image_dataset import get_dataset
    for i, e in enumerate((raster_golden["drop_edges"], raster_golden["graph0_edges"][:1200])):
        graph_io.write_csv(e, str(tmp_path / f"g{i}.csv"))
        Image.fromarray(np.random.RandomState(i).randint(0, 80, (304, 304)).astype(np.uint8)).save(str(tmp_path / f"b{i}.png"))
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "config_ves_seg-S_Menten_aug.yml")))
    csvs, pngs = str(tmp_path / "*.csv"), str(tmp_path / "*.png")
    cfg["Train"]["data"] = {"image": {"files": csvs}, "label": {"files": csvs}, "background": {"files": pngs}}
    cfg["Train"]["batch_size"] = 2
    cfg["General"].update(amp=False, seed=9)
    random.seed(1); np.random.seed(2); torch.manual_seed(3)
    loader = get_dataset(cfg, "Train", num_workers=0)
    assert loader.fused is None
    batches = list(loader)
    assert len(batches) == 1
    b = batches[0]
    for k in ("image", "label"):
        assert b[k].shape == (2, 1, 1216, 1216) and b[k].dtype == torch.float32 and b[k].is_cuda
    assert set(b["label"].unique().tolist()) <= {0.0, 1.0} and 0 <= b["image"].min().item() and b["image"].max().item() <= 1

    aug = cfg["Train"]["data_augmentation"]
    cut = [d["name"] for d in aug].index("MentenAugmentationd")
    items = loader.dataset.items
    got = {}
    for where in ("device", "host"):
        chain = T.get_data_augmentations(aug[:cut + 1], seed=9)
        random.seed(1); np.random.seed(2)
        got[where] = []
        for it in items:
            d = dict(it)
            for t in chain[:-1]:
                d = t(d)
            if where == "host":
                d = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in d.items()}
            d = chain[-1](d)
            got[where].append((d["image"].cpu(), d["label"].cpu()))
        got[where].append(np.random.uniform())
    for (ia, la), (ib, lb) in zip(got["device"][:2], got["host"][:2]):
        assert ia.shape == (1, 304, 304) and ia.dtype == ib.dtype == torch.float64 and la.shape == (1, 1216, 1216) and la.dtype == lb.dtype == torch.float32
        assert (ia - ib).abs().max().item() <= TOL and torch.equal(la, lb)
    assert got["device"][2] == got["host"][2]
