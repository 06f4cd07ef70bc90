"""GPU: the paper's noise model through csrc/noise_model.hip -- the fused pixel arithmetic against a float64 evaluation of the same formula,
the device-side Beta sampler against the Beta distribution, the counter-based generator's determinism, NoiseModeld and
RandomDecreaseResolutiond on CUDA samples, the loader and train.py on configs/config_ves_seg-S_RA.yml.

Measured on an MI355X (deterministic arithmetic, largest deviation from the float64 evaluation; torch's own float32 CPU evaluation beside it):
see DESIGN.md 4.2i."""
import os
import random
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

import _noise_model_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
N_DRAWS = 1 << 18
SIDE = 512                                               # 512 x 512 = 2^18 pixels: one draw per pixel and field
KS_BOUND = float(np.sqrt(np.log(2 / 1e-6) / (2 * N_DRAWS)))     # Dvoretzky-Kiefer-Wolfowitz at alpha = 1e-6: 0.0053
CORR_BOUND = 5 / np.sqrt(N_DRAWS)
LARGE_SHAPES = [(2, 2), (0.5, 0.5), (8, 1), (1, 8), (0.5, 3), (5, 0.5)]
SMALL_SHAPES = [(1e-3, 2), (2, 1e-3), (1e-3, 1e-3), (0.05, 0.05)]


@pytest.fixture(scope="module")
def dev(hip_lib_built):
    assert os.environ.get("OCTA_STRICT") == "1"          # tests/conftest.py: a host fallback of a supported layout would raise
    return torch.device("cuda", torch.cuda.current_device())


def constant_grids(pairs_v, pairs_s):
    """[B,5,9,9] control grids that are constant per map: sample b draws Delta ~ Beta(*pairs_v[b]) and N ~ Beta(*pairs_s[b]) at every pixel."""
    g = torch.full((len(pairs_v), 5, 9, 9), 0.5)
    for b, ((av, bv), (a_s, b_s)) in enumerate(zip(pairs_v, pairs_s)):
        for k, v in enumerate((av, bv, a_s, b_s)):
            g[b, k] = v
    return g


_FIELDS = {}


def drawn(dev, pair):
    """float64 numpy [SIDE, SIDE]: one field of 2^18 Beta(*pair) variates from the kernel, fixed seed; two pairs share a launch (Delta, N)."""
    from octa_autosegmentation_amd.data import gpu_augment
    pairs = LARGE_SHAPES + SMALL_SHAPES
    if pair not in _FIELDS:
        k = pairs.index(pair) // 2 * 2
        z = torch.zeros(1, SIDE, SIDE, device=dev)
        _, _, fields = gpu_augment.noise_model(z, z, constant_grids([pairs[k]], [pairs[k + 1]]), 0x5EED0000 + k, return_fields=True)
        _FIELDS[pairs[k]], _FIELDS[pairs[k + 1]] = (fields[0, f].cpu().numpy().astype(np.float64) for f in (0, 1))
    return _FIELDS[pair]


# ---- deterministic arithmetic ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape, names, lambdas", [((40, 56), ("a_0", "a_1", "c_0"), (1, 0.7, 0.3)), ((96, 128), ("b_0", "b_1", "a_0"), (0.8, 0.5, 0.2))])
def test_pixel_arithmetic_against_float64(dev, shape, names, lambdas):
    """Injected Delta and N: output and the five interpolated maps against torch's float64 CPU evaluation of the formula. Allowed: four times
    the largest deviation of torch's OWN float32 CPU evaluation from that float64 evaluation, per quantity (the kernel's pow and summation
    order differ from the CPU's by a few ulp). The control grids are ones the reference drew; their bicubic maps undershoot the 1e-3 clamp."""
    from octa_autosegmentation_amd.data import gpu_augment
    g = C.golden()
    gen = torch.Generator().manual_seed(shape[0])
    B = len(names)
    img, bg, delta, n = (torch.rand((B,) + shape, generator=gen) for _ in range(4))
    grids = torch.stack([torch.from_numpy(g[f"{k}_grids"].copy()) for k in names])
    out64, maps64, raw64 = C.evaluate(img, bg, grids, delta, n, lambdas, torch.float64)
    out32, maps32, _ = C.evaluate(img, bg, grids, delta, n, lambdas, torch.float32)
    assert raw64[:, :4].min().item() < 1e-3                  # the clamp is exercised
    out, maps, fields = gpu_augment.noise_model(img.to(dev), bg.to(dev), grids, 7, *lambdas, delta=delta.to(dev), n=n.to(dev), return_fields=True)
    assert out.dtype == torch.float32 and out.shape == (B,) + shape and maps.shape == (B, 5) + shape
    assert torch.equal(fields[:, 0].cpu(), delta) and torch.equal(fields[:, 1].cpu(), n)
    dev_err = lambda a, b: (a.cpu().double() - b).abs().max().item()
    for name, got, f32, f64 in [("out", out, out32, out64)] + [(f"map{k}", maps[:, k], maps32[:, k], maps64[:, k]) for k in range(5)]:
        ref_err, err = dev_err(f32, f64), dev_err(got, f64)
        print(f"[noise model {shape}] {name}: torch float32 vs float64 {ref_err:.3e}, kernel vs float64 {err:.3e}", flush=True)
        assert ref_err > 0 and err <= 4 * ref_err, (name, err, ref_err)
    assert maps[:, :4].min().item() == np.float32(1e-3)


# ---- the sampler -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", LARGE_SHAPES)
def test_sampler_ks_distance(dev, pair):
    from scipy import stats
    x = np.sort(drawn(dev, pair).ravel())
    assert x.size == N_DRAWS and np.isfinite(x).all() and x[0] >= 0 and x[-1] <= 1
    cdf = stats.beta.cdf(x, *pair)
    ks = max(np.max(np.arange(1, N_DRAWS + 1) / N_DRAWS - cdf), np.max(cdf - np.arange(N_DRAWS) / N_DRAWS))
    print(f"[sampler] Beta{pair}: KS distance {ks:.5f} (bound {KS_BOUND:.5f})", flush=True)
    assert ks <= KS_BOUND


@pytest.mark.parametrize("pair", SMALL_SHAPES)
def test_sampler_small_shapes_by_counts(dev, pair):
    """Shapes down to the clamp: the mass sits at values that underflow float32, so the fraction below 0.5 is tested, not a KS distance."""
    from scipy import stats
    x = drawn(dev, pair).ravel()
    assert x.size == N_DRAWS and np.isfinite(x).all() and x.min() >= 0 and x.max() <= 1
    frac, want = float((x < 0.5).mean()), float(stats.beta.cdf(0.5, *pair))
    print(f"[sampler] Beta{pair}: fraction below 0.5 {frac:.5f}, expected {want:.5f}", flush=True)
    assert abs(frac - want) <= 5 / (2 * np.sqrt(N_DRAWS))


def test_sampler_independence(dev):
    from octa_autosegmentation_amd.data import gpu_augment
    z = torch.zeros(2, SIDE, SIDE, device=dev)
    _, _, fields = gpu_augment.noise_model(z, z, constant_grids([(2, 2)] * 2, [(2, 2)] * 2), 99, return_fields=True)
    f = fields.cpu().numpy().astype(np.float64)
    corr = lambda a, b: float(np.corrcoef(a.ravel(), b.ravel())[0, 1])
    got = {"adjacent pixels": corr(f[0, 0][:, :-1], f[0, 0][:, 1:]), "Delta and N": corr(f[0, 0], f[0, 1]), "two samples": corr(f[0, 0], f[1, 0])}
    print(f"[sampler] correlations {got} (bound {CORR_BOUND:.5f})", flush=True)
    for what, c in got.items():
        assert abs(c) < CORR_BOUND, what


# ---- determinism -----------------------------------------------------------------------------------------------------------------

def test_counter_based_draws_are_reproducible(dev):
    from octa_autosegmentation_amd.data import gpu_augment
    g = C.golden()
    gen = torch.Generator().manual_seed(3)
    img, bg = torch.rand(3, 40, 56, generator=gen).to(dev), torch.rand(3, 40, 56, generator=gen).to(dev)
    grids = torch.stack([torch.from_numpy(g[f"{k}_grids"].copy()) for k in ("a_0", "a_1", "c_0")])
    seed = 0x0123456789ABCDEF
    out, maps, fields = gpu_augment.noise_model(img, bg, grids, seed, return_fields=True)
    again = gpu_augment.noise_model(img, bg, grids, seed, return_fields=True)
    assert torch.equal(out, again[0]) and torch.equal(fields, again[2])
    for bit in (0, 31, 32, 63):                              # both key words
        other = gpu_augment.noise_model(img, bg, grids, seed ^ (1 << bit), return_fields=True)[2]
        assert (other != fields).float().mean().item() > 0.9, bit
    # sample 1 of the batch = a launch of that sample alone under sample counter 1; under counter 0 it is another field
    one = gpu_augment.noise_model(img[1:2], bg[1:2], grids[1:2], seed, return_fields=True, sample_offset=1)
    assert torch.equal(one[0], out[1:2]) and torch.equal(one[2], fields[1:2]) and torch.equal(one[1], maps[1:2])
    assert not torch.equal(gpu_augment.noise_model(img[1:2], bg[1:2], grids[1:2], seed, return_fields=True)[2], fields[1:2])
    assert torch.isfinite(out).all() and fields.min().item() >= 0 and fields.max().item() <= 1


# ---- the transforms --------------------------------------------------------------------------------------------------------------

def test_noise_model_transform_on_a_cuda_sample(dev):
    from octa_autosegmentation_amd.data import data_transforms as T
    from octa_autosegmentation_amd.data.noise_model import NoiseModelDraws
    g = C.golden()
    res = C.run_case("b", dev)
    for out, _, d in res:
        assert out.is_cuda and out.dtype == torch.float32 and out.shape == (1, 96, 128) and torch.isfinite(out).all()
        assert np.array_equal(d["background"].cpu().numpy(), g["b_background"])
    # range [0, 1 + 1e-6], on an image in [0, 0.999]: then max(I, I_d Delta) (ls N + 1 - ls) + 1e-6 < 1, and Gamma > 0 (control values in
    # [0.7, 1.3], bicubic weights with an absolute sum <= 1.25^2), so the power is <= 1. At I = 1 and N = 1 the FORMULA gives (1 + 1e-6)^Gamma,
    # above 1 + 1e-6 wherever Gamma > 1: the reference's own output in the fixture (b_0_out) peaks at 1.0000011 on an image that reaches 1.0.
    random.seed(2); torch.manual_seed(2)
    t = T.NoiseModeld(["image"])
    for _ in range(2):
        out = t({"image": torch.from_numpy(g["b_in"] * np.float32(0.999)).to(dev), "background": torch.from_numpy(g["b_background"].copy()).to(dev)})["image"]
        assert out.is_cuda and out.dtype == torch.float32 and out.shape == (1, 96, 128)
        assert 0 <= out.min().item() and out.max().item() <= 1 + 1e-6 and torch.isfinite(out).all()
    # two instances after the same seeds agree bitwise; the control points are the host path's (= the reference's)
    again = C.run_case("b", dev)
    assert all(torch.equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(res, again))
    torch.manual_seed(int(g["b_seed"]))
    draws = NoiseModelDraws((9, 9))
    assert np.array_equal(torch.cat(draws.control_points(1), dim=1)[0].numpy(), g["b_0_grids"])
    # only the background term random: out >= img + 1e-6 up to rounding, with equality where the background is 0
    img, bg = torch.from_numpy(g["a_in"].copy()).to(dev), torch.from_numpy(g["a_background"].copy()).to(dev)
    bg[:, :, :20] = 0
    random.seed(1); torch.manual_seed(1)
    out = T.NoiseModeld(["image"], lambda_speckle=0, lambda_gamma=0)({"image": img, "background": bg})["image"]
    # "up to rounding": lambda_gamma = 0 makes the gamma grid the constant 1, whose bicubic map is the sum of 16 float32 weight products,
    # 1 within 16 ulp; pow(x, 1 + e) = x (1 + e ln x) with |ln x| <= 13.82 for x >= 1e-6; plus 4 ulp for powf and the additions
    rtol = (16 * 13.82 + 4) * 2.0 ** -24
    base = img + 1e-6
    assert (out >= base * (1 - rtol)).all() and (out > base * 1.01).any()
    assert torch.allclose(out[:, :, :20], base[:, :, :20], rtol=rtol, atol=0)


@pytest.mark.parametrize("what", ["two channels", "downsample_factor 2"])
def test_unsupported_cuda_layouts_report_the_host_path(dev, monkeypatch, what):
    from octa_autosegmentation_amd.data import data_transforms as T
    g = C.golden()
    img, bg = torch.from_numpy(g["a_in"].copy()).to(dev), torch.from_numpy(g["a_background"].copy()).to(dev)
    if what == "two channels":
        t, sample = T.NoiseModeld(["image"]), {"image": img.repeat(2, 1, 1), "background": bg.repeat(2, 1, 1)}
    else:
        # as in the reference, the background is NOT resampled: it has to come at the reduced size
        t, sample = T.NoiseModeld(["image"], downsample_factor=2), {"image": img, "background": bg[:, ::2, ::2].contiguous()}
    with pytest.raises(T.HostFallbackError, match="csrc/noise_model.hip"):
        t(sample)
    monkeypatch.setenv("OCTA_STRICT", "0")
    T._HOST_FALLBACK_WARNED.clear()
    with pytest.warns(RuntimeWarning, match="host restatement"):
        out = t(sample)["image"]
    assert out.is_cuda and out.shape == sample["image"].shape and torch.isfinite(out).all()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        t(sample)                                            # once


def _two_interpolations(x, factor):
    d = F.interpolate(x.unsqueeze(0), scale_factor=factor)
    return F.interpolate(d, size=x.shape[1:]).squeeze(0)


@pytest.mark.parametrize("size, count", [((37, 53), 200), ((304, 304), 20)])
def test_decrease_resolution_on_cuda_equals_cpu_interpolate(dev, monkeypatch, size, count):
    from octa_autosegmentation_amd.data import data_transforms as T
    x = torch.rand((1,) + size, generator=torch.Generator().manual_seed(size[0]))
    xd = x.to(dev)
    t = T.RandomDecreaseResolutiond(["image"])
    for f in np.linspace(0.25, 1.0, count).tolist():
        draws = iter([0.0, f])
        monkeypatch.setattr(random, "uniform", lambda a, b: next(draws))
        got = t({"image": xd})["image"]
        assert got.is_cuda and torch.equal(got.cpu(), _two_interpolations(x, f)), f


# ---- loader and train.py ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ra_files(tmp_path_factory, raster_golden, hip_lib_built):
    """Two short graphs from the raster fixture, two random background PNGs, and their rasters as validation / test PNGs."""
    from PIL import Image
    from octa_autosegmentation_amd import graph_io
    from octa_autosegmentation_amd.data import data_transforms as T
    tmp = tmp_path_factory.mktemp("ra")
    for sub in ("graphs", "background", "images", "labels"):
        os.makedirs(str(tmp / sub))
    load = T.LoadGraphAndFilterByRandomRadiusd(["image", "label"], image_resolutions=[[304, 304], [1216, 1216]], min_radius=[0, 0.0033])
    for i, e in enumerate((raster_golden["drop_edges"], raster_golden["graph0_edges"][:1200])):
        path = str(tmp / "graphs" / f"g{i}.csv")
        graph_io.write_csv(e, path)
        Image.fromarray(np.random.RandomState(i).randint(0, 80, (304, 304)).astype(np.uint8)).save(str(tmp / "background" / f"b{i}.png"))
        d = load({"image": path, "label": path})
        Image.fromarray(d["image"].cpu().numpy().astype(np.uint8)).save(str(tmp / "images" / f"{i}.png"))
        Image.fromarray(((d["label"] > 25).cpu().numpy() * 255).astype(np.uint8)).save(str(tmp / "labels" / f"{i}.png"))
    return tmp


def test_loader_with_the_ra_config(dev, ra_files):
    from octa_autosegmentation_amd.data.image_dataset import get_dataset
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "config_ves_seg-S_RA.yml")))
    csvs, pngs = str(ra_files / "graphs" / "*.csv"), str(ra_files / "background" / "*.png")
    cfg["Train"]["data"] = {"image": {"files": csvs}, "label": {"files": csvs}, "background": {"files": pngs}}
    cfg["Train"]["batch_size"] = 2
    cfg["General"].update(amp=False, seed=9)
    got = []
    for _ in range(2):
        random.seed(1); np.random.seed(2); torch.manual_seed(3)
        loader = get_dataset(cfg, "Train", num_workers=0)
        assert loader.fused is None and not loader.dataset.transform.batchable()
        batches = list(loader)
        assert len(batches) == 1
        got.append(batches[0])
    b = got[0]
    for k in ("image", "label"):
        assert b[k].shape == (2, 1, 1216, 1216) and b[k].dtype == torch.float32 and b[k].is_cuda and torch.isfinite(b[k]).all()
    assert set(b["label"].unique().tolist()) <= {0.0, 1.0}
    assert b["background"].shape == (2, 1, 304, 304)                      # NoiseModeld leaves the key in the sample
    assert torch.equal(got[0]["image"], got[1]["image"]) and torch.equal(got[0]["label"], got[1]["label"])
    assert b["image"].std().item() > 0.01 and not torch.equal(b["image"][0], b["image"][1])


def test_train_cli_with_the_ra_config(dev, ra_files, tmp_path):
    """One epoch of train.py --config_file configs/config_ves_seg-S_RA.yml under OCTA_STRICT=1: only paths, the epoch count and the seed are
    overridden (as tests/test_training_cli_gpu.py does for the S config)."""
    import train as train_cli
    assert os.environ.get("OCTA_STRICT") == "1"
    csvs = str(ra_files / "graphs" / "*.csv")
    f = lambda p: yaml.safe_dump({"files": p}, default_flow_style=True).strip()
    ov = ["--Train.data.image.files", csvs, "--Train.data.label.files", csvs, "--Train.data.background.files", str(ra_files / "background" / "*.png"),
          "--Train.epochs", "1", "--Train.epochs_decay", "0",
          "--Validation.data.image", f(str(ra_files / "images" / "*.png")), "--Validation.data.label", f(str(ra_files / "labels" / "*.png")),
          "--Test.data.image", f(str(ra_files / "images" / "*.png")), "--Output.save_dir", str(tmp_path / "results"), "--General.seed", "3"]
    run = train_cli.main(["--config_file", os.path.join(ROOT, "configs", "config_ves_seg-S_RA.yml")] + ov)
    rows = open(os.path.join(run, "metrics.csv")).read().splitlines()
    assert rows[0].startswith("epoch,train_DiceBCELoss") and len(rows) == 2
    vals = dict(zip(rows[0].split(","), (float(v) for v in rows[1].split(","))))
    assert np.isfinite(list(vals.values())).all() and 0 < vals["train_DiceBCELoss"] < 2
    assert "latest_model_model.pth" in os.listdir(os.path.join(run, "checkpoints"))
