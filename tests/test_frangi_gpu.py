"""GPU: the Frangi baseline (csrc/frangi.hip, models/frangi.py) against the fixtures (tests/golden/frangi_golden*.npz,
tools/make_golden_frangi.py) -- Hessian planes, sorted eigenvalues and gamma bit for bit, the vesselness within 2^-20 --, batch /
run-to-run bit identity, and test.py / validate.py on configs/config_frangi.yml end to end.

The output bound: up to the two exp calls the kernel is bit-identical to the reference; E and T may each differ from numpy's
float32 exp by a few ulps at 1, budgeted as 4 * 2^-24 each, so E T differs by at most 2 * 4 * 2^-24 = 2^-21; doubled, 2^-20.
A wrong tap, sign, scale or gamma is off by 1e-3 or more."""
import hashlib
import os

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

from octa_autosegmentation_amd.models import frangi as frangi_mod

from test_frangi import CASES, PLANES, SCALES, TINY
from test_oof import CASES as OOF_CASES, ROOT
from test_oof_gpu import _post, _write_dataset

pytestmark = pytest.mark.gpu

OUT_TOL = 2.0 ** -20


def _input(name):
    return torch.from_numpy(CASES[name]["img"]).cuda()[None, None]


def _sha(plane):
    return hashlib.sha256(np.ascontiguousarray(plane + np.float32(0.0)).tobytes()).hexdigest().encode()


@pytest.mark.parametrize("name", sorted(CASES))
def test_hessian_eigenvalues_and_gamma_are_bit_identical(name, hip_lib_built):
    c = CASES[name]
    img, f, st = _input(name), frangi_mod.Frangi(), int(c["step"])
    for s, sigma in enumerate(SCALES):
        H = f.hessian(img, sigma)
        l1, l2, gamma = f.eigenvalues(img, sigma)
        assert gamma.dtype == torch.float32 and gamma.shape == (1,)
        if s == 0:
            assert gamma.cpu().numpy()[0].tobytes() == c["gamma"].tobytes()
        for i, (k, t) in enumerate(zip(PLANES, H + (l1, l2))):
            assert t.dtype == torch.float32 and t.shape == img.shape
            got = t[0, 0].cpu().numpy()
            assert np.array_equal(got[::st, ::st], c[f"s{s}_{k}"]), (name, sigma, k)
            assert _sha(got) == c[f"s{s}_sha"][i], (name, sigma, k)
    if "tie_idx" in c:
        for s, sigma in enumerate(SCALES):
            l1, l2, _ = f.eigenvalues(img, sigma)
            sel = c["tie_idx"][:, 0] == s
            y, x = c["tie_idx"][sel, 1], c["tie_idx"][sel, 2]
            assert np.array_equal(l1[0, 0].cpu().numpy()[y, x], c["tie_l1"][sel]) and np.array_equal(l2[0, 0].cpu().numpy()[y, x], c["tie_l2"][sel])


@pytest.mark.parametrize("name", sorted(CASES))
def test_frangi_matches_reference(name, hip_lib_built):
    c = CASES[name]
    img = _input(name)
    out = frangi_mod.Frangi()(img)
    assert out.dtype == torch.float64 and out.shape == img.shape
    out = out[0, 0].cpu().numpy()
    st = int(c["outstep"])
    err = np.abs(out[::st, ::st] - c["out"]).max()
    print(f"{name}: max |out - fixture| = {err:.3g}")
    assert err <= OUT_TOL
    if "tie_idx" in c:
        terr = np.abs(out[c["tie_idx"][:, 1], c["tie_idx"][:, 2]] - c["tie_out"]).max()
        print(f"{name}: max error at the {len(c['tie_idx'])} tie pixels = {terr:.3g}")
        assert terr <= OUT_TOL
    if name in ("t1x1", "const"):
        assert not out.any()
    if name == "full":
        for k, v in (("out_max", out.max()), ("out_min", out.min()), ("out_sum", out.sum())):
            print(f"full {k}: {v!r} (fixture {float(c[k])!r})")
            assert abs(v - float(c[k])) <= OUT_TOL * abs(float(c[k])), k


def test_general_entry_point_equals_the_model(hip_lib_built):
    img = _input("odd")
    ref = frangi_mod.Frangi()(img)
    a = img * 255
    assert torch.equal(frangi_mod.frangi_2d(a, sigmas=(0.5, 2, 0.5), beta=15, black_ridges=False), ref)
    assert torch.equal(frangi_mod.frangi_2d(a, sigmas=(0.5, 2), beta=15, black_ridges=False), ref)
    # a fixed gamma equal to the image's own gives the same 2 gamma^2 here: gamma^2 is exact in double, rounded to float32 once
    gamma = float(CASES["odd"]["gamma"])
    fixed = frangi_mod.frangi_2d(a, sigmas=(0.5, 2), beta=15, gamma=gamma, black_ridges=False)
    assert (fixed - ref).abs().max().item() <= OUT_TOL
    # dark ridges of the negated image are the bright ridges of the image
    assert torch.equal(frangi_mod.frangi_2d(-a, sigmas=(0.5, 2), beta=15, black_ridges=True), ref)


def test_frangi_batch_equals_single_runs_bit_for_bit(hip_lib_built):
    rng = np.random.default_rng(5)
    imgs = torch.from_numpy(rng.integers(0, 256, (4, 1, 76, 90)).astype(np.float32) / np.float32(255)).cuda()
    f = frangi_mod.Frangi()
    batch = f(imgs)
    assert torch.equal(batch, f(imgs))
    singles = [f(imgs[i:i + 1].contiguous()) for i in range(4)]
    for i in range(4):
        assert torch.equal(batch[i:i + 1], singles[i])
    assert not torch.equal(singles[0], singles[1])


def test_invalid_arguments_are_refused(hip_lib_built):
    from octa_autosegmentation_amd import _native
    x = torch.zeros(1, 1, 8, 8, device="cuda")
    with pytest.raises(_native.OctaHipError, match="non-zero taps"):
        frangi_mod.frangi_2d(x, sigmas=(40,))           # 226 taps per side
    with pytest.raises(ValueError):
        frangi_mod.frangi_2d(x, sigmas=tuple(range(1, 11)))
    with pytest.raises(ValueError):
        frangi_mod.frangi_2d(x, gamma=0.0)
    with pytest.raises(TypeError):
        frangi_mod.Frangi()(x.double())


def test_test_and_validate_cli_end_to_end(tmp_path, hip_lib_built):
    import test as test_cli
    import validate as validate_cli
    from octa_autosegmentation_amd.data.image_dataset import get_dataset, get_post_transformation
    from octa_autosegmentation_amd.utils.config_overrides import apply_cli_overrides_from_unknown_args
    from octa_autosegmentation_amd.utils.enums import Phase
    from octa_autosegmentation_amd.utils.metrics import MetricsManager
    cfg_path = os.path.join(ROOT, "configs", "config_frangi.yml")
    with open(cfg_path) as f:
        config = yaml.safe_load(f)
    common = ["--General.device", "cuda:0", "--Output.save_dir", str(tmp_path / "out")]

    # Test phase (threshold 0.04, min_size 5): octa and even keep their margins and objects there (tools/make_golden_frangi.py)
    names = ["octa", "even"]
    (tmp_path / "t").mkdir()
    images, labels, split = _write_dataset(tmp_path / "t", names)
    test_dir = tmp_path / "test"
    written = test_cli.main(["--config_file", cfg_path, "--num_workers", "0", "--Test.data.image.files", str(images / "*.png"),
                             "--Test.data.image.split", str(split), "--Test.save_dir", str(test_dir)] + common)
    assert len(written) == 2
    for i, name in enumerate(names):
        expect = (_post(config, Phase.TEST, CASES[name]["out"])[0].float().cpu().numpy() * 255).astype(np.uint8)
        got = np.asarray(Image.open(test_dir / f"pred_img_{i}.png"))
        assert expect.any() and got.shape == (1216, 1216) and np.array_equal(got, expect), name

    # Validation phase (threshold 0.75, min_size 31): only octa holds there, so it is written twice
    names = ["octa", "octa"]
    (tmp_path / "v").mkdir()
    images, labels, split = _write_dataset(tmp_path / "v", names)
    ov = ["--Validation.data.image.files", str(images / "*.png"), "--Validation.data.image.split", str(split),
          "--Validation.data.label.files", str(labels / "*.png"), "--Validation.data.label.split", str(split)]
    metrics = validate_cli.main(["--config_file", cfg_path, "--num_workers", "0"] + ov + common)

    # the same metrics from the fixture's outputs, through the same post-processing on the GPU
    apply_cli_overrides_from_unknown_args(config, ov + common)
    loader = get_dataset(config, Phase.VALIDATION, num_workers=0)
    mm = MetricsManager(Phase.VALIDATION)
    label_post = get_post_transformation(config, Phase.VALIDATION)["label"]
    for i, batch in enumerate(loader):
        pred = _post(config, Phase.VALIDATION, CASES[names[i]]["out"])
        assert pred.any()
        mm([pred], [label_post(batch["label"][0].to("cuda:0"))])
    loader.close()
    expect = {k: float(str(round(v, 3))) for k, v in mm.aggregate_and_reset(Phase.VALIDATION).items()}
    assert metrics and metrics == expect
