"""GPU: the grey-level area opening / closing (csrc/morph.hip) against the CPU references of tests/_morph_ref.py on the smallest
planes that can go wrong, the whole sketch filter (models/skrgan.py) against the fixture (tests/golden/skrgan_golden.npz,
tools/make_golden_skrgan.py) plane by plane, batch / run-to-run bit identity, sentinels around the output, and test.py /
validate.py on configs/config_skrgan.yml end to end. Every comparison is exact."""
import os

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

from octa_autosegmentation_amd import _native
from octa_autosegmentation_amd.models import skrgan as skr_mod

from _guarded import Guarded
from _morph_ref import closing, uf_opening
from test_oof import ROOT
from test_oof_gpu import _post, _write_dataset
from test_skrgan import CASES, LAMBDAS, NAN_FROM, PLANES, np_sketch, plateau_plane, quantised, same, sha

pytestmark = pytest.mark.gpu


def gpu_open(f, lam):
    return skr_mod.area_opening(torch.from_numpy(np.ascontiguousarray(f)).cuda(), lam).cpu().numpy()


def gpu_close(f, lam):
    return skr_mod.area_closing(torch.from_numpy(np.ascontiguousarray(f)).cuda(), lam).cpu().numpy()


def two_hills_and_a_saddle():
    """Hills of 5 and 6 pixels joined by a saddle above the ground: with lambda = 17 both come down to the ground, and only the
    lower hill's own growth, which has to climb the higher hill, lowers the lower hill."""
    f = np.zeros((8, 12), np.float32)
    f[2:4, 1:3], f[4, 1] = 3, 3                 # the lower hill, 5 pixels
    f[3, 3:5] = 2                               # the saddle
    f[2:5, 5:7] = 5                             # the higher hill, 6 pixels
    return f


def small_hill_beside_a_large_hill():
    """A hill of 4 pixels whose saddle leads onto a hill of 30: with lambda = 17 the small hill comes down to the saddle and the
    large hill, which the small hill's growth spills onto, does not change."""
    f = np.zeros((9, 14), np.float32)
    f[3:5, 1:3] = 5                             # the small hill
    f[4, 3:5] = 2                               # the saddle
    f[2:7, 5:11] = 4                            # the large hill
    return f


def plateau(n, shape=(20, 20)):
    """a maximal plateau of n pixels on a sloping ground"""
    f = (np.add.outer(np.arange(shape[0]), np.arange(shape[1])) / np.float32(1000)).astype(np.float32)
    f.ravel()[np.arange(n) % 11 + (np.arange(n) // 11 + 2) * shape[1] + 3] = 1        # rows of 11 from (2, 3)
    return f


def test_images_of_exactly_lambda_pixels_and_just_above():
    rng = np.random.default_rng(1)
    for shape in ((8, 8), (1, 64), (64, 1)):
        f = rng.random(shape).astype(np.float32)
        got = gpu_open(f, 64)
        assert np.array_equal(got, np.full(shape, f.min())) and np.array_equal(got, uf_opening(f, 64))
    for shape in ((1, 65), (9, 8), (65, 1), (1, 129), (13, 10)):
        for f in (rng.random(shape).astype(np.float32), quantised(rng, shape, 3)):
            for lam in (64, 65, 128):
                if f.size >= lam:
                    assert np.array_equal(gpu_open(f, lam), uf_opening(f, lam)), (shape, lam)
    for shape in ((2, 4096), (4096, 1)):        # the largest coordinates the packed positions hold
        f = quantised(rng, shape, 6)
        assert np.array_equal(gpu_open(f, 65), uf_opening(f, 65)), shape
        assert np.array_equal(gpu_close(f, 64), closing(f, 64)), shape


def test_the_two_traps():
    f = two_hills_and_a_saddle()
    got = gpu_open(f, 17)
    assert np.array_equal(got, uf_opening(f, 17)) and not got.any()             # the lower hill is lowered too
    assert np.array_equal(gpu_open(f, 13), np.minimum(f, 2))                     # both hills and the saddle are 13 pixels
    f = small_hill_beside_a_large_hill()
    got = gpu_open(f, 17)
    assert np.array_equal(got, uf_opening(f, 17))
    assert (got[3:5, 1:3] == 2).all() and np.array_equal(got[2:7, 5:11], f[2:7, 5:11])     # the large hill does not change
    for g in (f, two_hills_and_a_saddle()):
        for lam in LAMBDAS[:6]:
            assert np.array_equal(gpu_open(g, lam), uf_opening(g, lam)), lam


def test_plateaus_constant_checkerboard_and_identity():
    for lam in (64, 128):
        below, at = plateau(lam - 1), plateau(lam)
        got = gpu_open(at, lam)
        assert (got[at == 1] == 1).all() and np.array_equal(got, uf_opening(at, lam))
        got = gpu_open(below, lam)
        assert got.max() < 1 and np.array_equal(got, uf_opening(below, lam))
    const = np.full((23, 31), np.float32(0.375))
    checker = ((np.add.outer(np.arange(17), np.arange(19)) % 2) * np.float32(0.75) + np.float32(0.125)).astype(np.float32)
    rng = np.random.default_rng(2)
    smooth = rng.random((17, 19)).astype(np.float32)
    for lam in LAMBDAS:
        assert np.array_equal(gpu_open(const, lam), const)
        assert np.array_equal(gpu_open(checker, lam), checker if lam == 1 else np.full_like(checker, 0.125)), lam
    assert np.array_equal(gpu_open(smooth, 1), smooth) and np.array_equal(gpu_close(smooth, 1), np.float32(1) - (np.float32(1) - smooth))
    neg = smooth - np.float32(0.5)              # the opening takes any finite values
    assert np.array_equal(gpu_open(neg, 17), uf_opening(neg, 17))


@pytest.mark.parametrize("shape", [(17, 19), (64, 48)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_quantised_and_plateau_planes_for_every_lambda(shape):
    rng = np.random.default_rng(shape[0])
    planes = [quantised(rng, shape, 3), quantised(rng, shape, 6), plateau_plane(rng, shape)]
    for i, f in enumerate(planes):
        for lam in LAMBDAS:
            ref = uf_opening(f, lam)
            assert np.array_equal(gpu_open(f, lam), ref), (i, lam)
            if lam in (5, 64, 65):
                assert np.array_equal(gpu_close(f, lam), closing(f, lam)), (i, lam)


def test_smooth_random_plane_and_its_closing():
    rng = np.random.default_rng(3)
    f = rng.random((91, 97)).astype(np.float32)
    from scipy import ndimage as ndi
    f = ndi.uniform_filter(f, 5).astype(np.float32)         # hills of a few dozen pixels: the regions cross every 64-pixel chunk
    for lam in (17, 64, 128):
        ref = uf_opening(f, lam)
        assert (ref != f).sum() > 100
        assert np.array_equal(gpu_open(f, lam), ref), lam
        assert np.array_equal(gpu_close(f, lam), closing(f, lam)), lam


def test_batch_equals_single_runs_reruns_and_sentinels():
    rng = np.random.default_rng(4)
    imgs = torch.from_numpy(np.stack([rng.random((37, 41)).astype(np.float32), quantised(rng, (37, 41), 6), plateau_plane(rng, (37, 41))])).cuda()[:, None]
    for fn in (skr_mod.area_opening, skr_mod.area_closing, skr_mod.sketch_filter):
        batch = fn(imgs)
        assert batch.shape == imgs.shape and batch.dtype == torch.float32
        assert torch.equal(batch, fn(imgs))
        for i in range(3):
            assert torch.equal(batch[i:i + 1], fn(imgs[i:i + 1].contiguous())), (fn.__name__, i)
        assert not torch.equal(batch[0], batch[1])
    assert np.array_equal(skr_mod.area_opening(imgs)[1, 0].cpu().numpy(), uf_opening(imgs[1, 0].cpu().numpy(), 64))
    # the native calls between sentinels, at an odd offset
    x = imgs[:, 0].contiguous()
    b, h, w = x.shape
    ws = torch.empty(_native.lib().octa_skr_workspace_bytes(b, h, w), dtype=torch.uint8, device="cuda")
    for closing_flag in (0, 1):
        out = Guarded(x.shape, torch.float32, offset=3)
        _native.call("octa_area_opening", x, out.t, b, h, w, 65, closing_flag, ws, _native.current_stream_ptr())
        torch.cuda.synchronize()
        assert out.intact() and out.unwritten() == 0
        assert torch.equal(out.t, (skr_mod.area_closing if closing_flag else skr_mod.area_opening)(x, 65))
    planes = [Guarded(x.shape, torch.float32, offset=1) for _ in range(4)]
    wt = skr_mod.gaussian_weights(2)
    _native.call("octa_skr_filter", x, *[p.t for p in planes], b, h, w, 8, wt.ctypes.data, 64, 64, ws, _native.current_stream_ptr())
    torch.cuda.synchronize()
    assert all(p.intact() and p.unwritten() == 0 for p in planes)
    assert torch.equal(planes[3].t, skr_mod.sketch_filter(x))


@pytest.mark.parametrize("name", sorted(CASES))
def test_stage_planes_match_the_fixture(name):
    c = CASES[name]
    img = torch.from_numpy(c["img"]).cuda()[None, None]
    f = skr_mod.SkrGAN()
    stages = f.stages(img)
    st = int(c["step"])
    for i, (k, t) in enumerate(zip(PLANES, stages)):
        assert t.dtype == torch.float32 and t.shape == img.shape and t.is_cuda
        got = t[0, 0].cpu().numpy()
        full = k == "out" and c[k].shape == got.shape
        assert same(got if full else got[::st, ::st], c[k]), (name, k)
        assert sha(got) == c["sha"][i], (name, k)
        assert np.isnan(got).all() == (name in NAN_FROM and i >= NAN_FROM[name]) and np.isnan(got).all() == np.isnan(got).any()
    assert torch.equal(f(img), stages[3]) or name in NAN_FROM


def test_constant_image_is_all_nan_and_does_not_disturb_its_batch():
    const = torch.full((1, 1, 9, 9), 9 / 255, device="cuda")
    assert all(torch.isnan(p).all() for p in skr_mod.SkrGAN().stages(const))
    img = torch.from_numpy(CASES["r20x23"]["img"]).cuda()[None, None]
    batch = torch.cat([img, torch.full_like(img, 0.5), img])
    out = skr_mod.SkrGAN()(batch)
    assert torch.isnan(out[1]).all() and torch.equal(out[0], out[2]) and same(out[0, 0].cpu().numpy(), CASES["r20x23"]["out"])


def test_arguments_are_honoured_by_the_function_and_ignored_by_the_class():
    c = CASES["odd"]
    img = torch.from_numpy(c["img"]).cuda()[None, None]
    ref = skr_mod.SkrGAN()(img)
    assert torch.equal(skr_mod.sketch_filter(img), ref) and torch.equal(skr_mod.sketch_filter(img, 2, 64, 64), ref)
    assert torch.equal(skr_mod.SkrGAN(2, 5, 2, 7, 2)(img), ref)                 # the reference's quirk
    got = skr_mod.sketch_stages(img, 2, 68, 86)                                 # the notebook's thresholds
    want = np_sketch(c["img"], 2, 68, 86)
    for k, t, r in zip(PLANES, got, want):
        assert same(t[0, 0].cpu().numpy(), r), k
    assert not torch.equal(got[3], ref)
    got = skr_mod.sketch_stages(img, 0, 64, 64)                                 # sigma 0: scipy copies
    want = np_sketch(c["img"], 0, 64, 64)
    assert torch.equal(got[0], got[1])
    for k, t, r in zip(PLANES, got, want):
        assert same(t[0, 0].cpu().numpy(), r), k
    got = skr_mod.SkrGAN(sigma=1)(img)                                          # another sigma: the table is built at run time
    assert same(got[0, 0].cpu().numpy(), np_sketch(c["img"], 1)[3])


def test_invalid_arguments_are_refused():
    x = torch.zeros(1, 1, 8, 8, device="cuda")
    with pytest.raises(_native.OctaHipError, match="non-zero taps"):
        skr_mod.sketch_filter(x, sigma=40)
    with pytest.raises(TypeError):
        skr_mod.SkrGAN()(x.double())
    with pytest.raises(ValueError):
        skr_mod.area_opening(x, 65)
    with pytest.raises(ValueError):
        skr_mod.area_opening(x, 64, connectivity=2)
    with pytest.raises(ValueError):
        skr_mod.sketch_filter(x, sigma=-1)


def test_test_and_validate_cli_end_to_end(tmp_path, hip_lib_built):
    import test as test_cli
    import validate as validate_cli
    from octa_autosegmentation_amd.data.image_dataset import get_dataset, get_post_transformation
    from octa_autosegmentation_amd.utils.config_overrides import apply_cli_overrides_from_unknown_args
    from octa_autosegmentation_amd.utils.enums import Phase
    from octa_autosegmentation_amd.utils.metrics import MetricsManager
    assert os.environ.get("OCTA_STRICT") == "1"
    cfg_path = os.path.join(ROOT, "configs", "config_skrgan.yml")
    with open(cfg_path) as f:
        config = yaml.safe_load(f)
    common = ["--General.device", "cuda:0", "--Output.save_dir", str(tmp_path / "out")]
    names = ["octa", "even"]
    images, labels, split = _write_dataset(tmp_path, names)

    test_dir = tmp_path / "test"
    written = test_cli.main(["--config_file", cfg_path, "--num_workers", "0", "--Test.data.image.files", str(images / "*.png"),
                             "--Test.data.image.split", str(split), "--Test.save_dir", str(test_dir)] + common)
    assert len(written) == 2
    for i, name in enumerate(names):
        expect = (_post(config, Phase.TEST, CASES[name]["out"])[0].float().cpu().numpy() * 255).astype(np.uint8)
        got = np.asarray(Image.open(test_dir / f"pred_img_{i}.png"))
        assert expect.any() and got.shape == (1216, 1216) and np.array_equal(got, expect), name

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
