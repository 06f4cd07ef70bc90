"""GPU: the OOF baseline (csrc/oof.hip, models/oof.py) -- its complex-double FFT against numpy.fft, the filter against the
reference's own outputs (tests/golden/oof_golden*.npz, tools/make_golden_oof.py), batch / run-to-run bit identity, and
test.py / validate.py on configs/config_oof.yml end to end."""
import os

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

from octa_autosegmentation_amd.models import oof as oof_mod

from test_oof import CASES, ROOT

pytestmark = pytest.mark.gpu

FFT_SHAPES = [(1, 1), (2, 2), (3, 3), (5, 5), (7, 7), (16, 16), (19, 19), (91, 97), (128, 128), (304, 304), (400, 400),
              (1216, 1216), (1217, 1217), (48, 1216)]


@pytest.mark.parametrize("shape", FFT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("b", [1, 3])
def test_fft2_matches_numpy(shape, b, hip_lib_built):
    rng = np.random.default_rng(shape[0] * 7919 + shape[1] * 31 + b)
    x = rng.standard_normal((b,) + shape) + 1j * rng.standard_normal((b,) + shape)
    xd = torch.from_numpy(x).cuda()
    for inverse, ref in ((False, np.fft.fft2(x)), (True, np.fft.ifft2(x))):
        got = oof_mod.fft2_c2c_f64(xd, inverse=inverse).cpu().numpy()
        err = np.abs(got - ref).max()
        assert err <= 1e-12 * np.abs(ref).max(), (shape, b, inverse, err)


def _input(name):
    return torch.from_numpy(CASES[name]["img"]).cuda()[None, None]


@pytest.mark.parametrize("name", sorted(CASES))
def test_oof_matches_reference(name, hip_lib_built):
    c = CASES[name]
    img = _input(name)
    out = oof_mod.OOF()(img)
    raw = oof_mod.OOF().response(img)
    assert out.dtype == torch.float64 and out.shape == img.shape
    out, raw = out[0, 0].cpu().numpy(), raw[0, 0].cpu().numpy()
    s = c["step"]
    got_out = out if c["out"].shape == out.shape else out[::s, ::s]
    assert np.abs(got_out - c["out"]).max() <= 1e-12
    assert np.abs(raw[::s, ::s] - c["raw"]).max() <= 1e-12 * float(c["raw_absmax"])
    if name == "full":
        for k, v in (("out_max", out.max()), ("out_min", out.min()), ("out_sum", out.sum())):
            assert abs(v - float(c[k])) <= 1e-12 * abs(float(c[k])), k


def test_oof_batch_equals_single_runs_bit_for_bit(hip_lib_built):
    rng = np.random.default_rng(5)
    imgs = torch.from_numpy(rng.integers(0, 256, (4, 1, 76, 90)).astype(np.float32) / np.float32(255)).cuda()
    f = oof_mod.OOF()
    batch = f(imgs)
    assert torch.equal(batch, f(imgs))
    for i in range(4):
        assert torch.equal(batch[i:i + 1], f(imgs[i:i + 1].contiguous()))


def _write_dataset(tmp_path, names):
    """PNG images of fixture cases (the loading transforms give back exactly the fixture's input) and labels; split files."""
    images, labels = tmp_path / "images", tmp_path / "labels"
    images.mkdir()
    labels.mkdir()
    for i, name in enumerate(names):
        c = CASES[name]
        u8 = c["u8"]
        assert u8.min() == 0 and float(u8.max()) == float(c["div"])     # ScaleIntensityd divides by the maximum
        Image.fromarray(u8).save(images / f"img_{i}.png")
        Image.fromarray(((u8 > 100) * 255).astype(np.uint8)).save(labels / f"img_{i}.png")
    split = tmp_path / "split.txt"
    split.write_text("".join(f"{i}\n" for i in range(len(names))))
    return images, labels, split


def _post(config, phase, ref_out):
    from octa_autosegmentation_amd.data.image_dataset import get_post_transformation
    return get_post_transformation(config, phase)["prediction"](torch.from_numpy(ref_out).cuda()[None])


def test_test_and_validate_cli_end_to_end(tmp_path, hip_lib_built):
    import test as test_cli
    import validate as validate_cli
    from octa_autosegmentation_amd.data.image_dataset import get_dataset, get_post_transformation
    from octa_autosegmentation_amd.utils.enums import Phase
    from octa_autosegmentation_amd.utils.metrics import MetricsManager
    names = ["octa", "even"]
    images, labels, split = _write_dataset(tmp_path, names)
    cfg_path = os.path.join(ROOT, "configs", "config_oof.yml")
    with open(cfg_path) as f:
        config = yaml.safe_load(f)
    out_dir = tmp_path / "out"
    common = ["--General.device", "cuda:0", "--Output.save_dir", str(out_dir)]

    test_dir = tmp_path / "test"
    written = test_cli.main(["--config_file", cfg_path, "--num_workers", "0", "--Test.data.image.files", str(images / "*.png"),
                             "--Test.data.image.split", str(split), "--Test.save_dir", str(test_dir)] + common)
    assert len(written) == 2
    for i, name in enumerate(names):
        expect = (_post(config, Phase.TEST, CASES[name]["out"])[0].float().cpu().numpy() * 255).astype(np.uint8)
        got = np.asarray(Image.open(test_dir / f"pred_img_{i}.png"))
        assert got.shape == (1216, 1216) and np.array_equal(got, expect), name

    ov = ["--Validation.data.image.files", str(images / "*.png"), "--Validation.data.image.split", str(split),
          "--Validation.data.label.files", str(labels / "*.png"), "--Validation.data.label.split", str(split)]
    metrics = validate_cli.main(["--config_file", cfg_path, "--num_workers", "0"] + ov + common)

    # the same metrics from the reference's outputs, through the same post-processing on the GPU
    from octa_autosegmentation_amd.utils.config_overrides import apply_cli_overrides_from_unknown_args
    apply_cli_overrides_from_unknown_args(config, ov + common)
    loader = get_dataset(config, Phase.VALIDATION, num_workers=0)
    mm = MetricsManager(Phase.VALIDATION)
    label_post = get_post_transformation(config, Phase.VALIDATION)["label"]
    for i, batch in enumerate(loader):
        mm([_post(config, Phase.VALIDATION, CASES[names[i]]["out"])], [label_post(batch["label"][0].to("cuda:0"))])
    loader.close()
    expect = {k: float(str(round(v, 3))) for k, v in mm.aggregate_and_reset(Phase.VALIDATION).items()}
    assert metrics and metrics == expect

