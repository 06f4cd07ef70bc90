"""GPU: the skeletonisation kernel (csrc/skeleton.hip through utils/skeleton.py) bit for bit against the literal oracle of
tests/test_skeleton.py and, at 1216 x 1216, against skeletonize_host; batches, input forms, the aliasing check, ClDiceMetric on the
device against the reference's recorded scores, and validate.py end to end with its Validation_ClDice column."""
import ctypes
import os

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

from octa_autosegmentation_amd import _native
from octa_autosegmentation_amd.utils.skeleton import skeletonize_device, skeletonize_host

from test_skeleton import GOLDEN, KNOWN, ROOT, check_metric_against_golden, oracle, oracle_of, random_mask

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 6), (2, 2), (9, 9), (63, 65), (64, 64), (65, 63), (97, 131)]      # word seams at 64, widths that are no multiple of it


def _device(mask):
    out, passes = skeletonize_device(torch.from_numpy(np.ascontiguousarray(mask)).cuda(), return_passes=True)
    assert out.dtype == torch.uint8 and out.is_cuda and out.shape == mask.shape
    return out.cpu().numpy(), passes


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_the_literal_oracle(shape, hip_lib_built):
    h, w = shape
    masks = [(f"random_{h}_{w}_{d}", random_mask(shape, d / 100)) for d in (35, 50, 62)]
    masks.append(("full97x131" if shape == (97, 131) else None, np.ones(shape, np.uint8)))
    masks.append((None, np.zeros(shape, np.uint8)))
    for name, mask in masks:
        ref, removing = oracle_of(name) if name else oracle(mask)
        got, passes = _device(mask)
        assert np.array_equal(got, ref), (shape, name)
        assert passes == removing + 1, (shape, name)              # the removing double passes and the one that found nothing


@pytest.mark.parametrize("name", ["3x7", "5x5", "8x8", "disc", "recalled_ellipse"])
def test_kernel_known_answers(name, hip_lib_built):
    mask, expect, count = KNOWN[name]
    got, passes = _device(mask)
    ref, removing = oracle_of(name)
    assert np.array_equal(got, ref) and int(got.sum()) == count and passes == removing + 1
    if expect is not None:
        assert np.array_equal(got, expect)


def test_kernel_lines_on_word_seams(hip_lib_built):
    for x in (31, 32, 63, 64):
        mask = np.zeros((97, 131), np.uint8)
        mask[:, x] = 1
        ref, _ = oracle(mask)
        assert np.array_equal(_device(mask)[0], ref) and np.array_equal(ref, mask), x
        mask[:, x + 1] = 1                                         # two pixels wide across the seam: really thinned
        ref, _ = oracle(mask)
        assert np.array_equal(_device(mask)[0], ref) and ref.sum() < mask.sum(), x
    mask = np.zeros((97, 131), np.uint8)
    mask[-1, :] = 1
    ref, _ = oracle(mask)
    assert np.array_equal(_device(mask)[0], ref) and np.array_equal(ref, mask)
    mask[-3:, :] = 1
    ref, _ = oracle(mask)
    assert np.array_equal(_device(mask)[0], ref)


def test_batch_equals_single_runs(hip_lib_built):
    imgs = [np.ones((97, 131), np.uint8), np.zeros((97, 131), np.uint8), random_mask((97, 131), 0.5)]
    singles = [_device(m)[0] for m in imgs]
    assert np.array_equal(singles[0], oracle_of("full97x131")[0]) and np.array_equal(singles[2], oracle_of("random_97_131_50")[0])
    batch, passes = _device(np.stack(imgs))
    assert passes == 49                                            # the slowest image's
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0), (2, 1, 0)):
        got, _ = _device(np.stack([imgs[i] for i in order]))
        for k, i in enumerate(order):
            assert np.array_equal(got[k], singles[i]), order
    assert np.array_equal(_device(np.stack(imgs))[0], batch)


def test_wrapper_input_forms_and_aliasing(hip_lib_built):
    mask = random_mask((65, 63), 0.5)
    ref = oracle_of("random_65_63_50")[0]
    m = torch.from_numpy(mask).cuda()
    assert np.array_equal(skeletonize_device(m).cpu().numpy(), ref)
    assert np.array_equal(skeletonize_device(m.bool()).cpu().numpy(), ref)
    assert np.array_equal(skeletonize_device(m * 200).cpu().numpy(), ref)
    assert np.array_equal(skeletonize_device(m.float() * -0.25).cpu().numpy(), ref)
    wide = torch.zeros(65, 126, dtype=torch.float32, device="cuda")
    wide[:, ::2] = m.float() * 3
    view = wide[:, ::2]
    assert not view.is_contiguous()
    assert np.array_equal(skeletonize_device(view).cpu().numpy(), ref)
    assert np.array_equal(skeletonize_device(m.t().contiguous().t()).cpu().numpy(), ref)
    with pytest.raises(RuntimeError):
        skeletonize_device(m.cpu())
    with pytest.raises(NotImplementedError):
        skeletonize_device(m[None, None])

    lib, p = _native.lib(), ctypes.c_void_p(m.data_ptr())
    before = m.clone()
    rc = lib.octa_skeletonize(_native.ctx(m.device.index), p, 1, 65, 63, p, None, _native.current_stream_ptr())
    assert rc == -2 and b"alias" in lib.octa_last_error()
    both = torch.zeros(2, 65, 63, dtype=torch.uint8, device="cuda")         # a partial overlap is refused as well
    rc = lib.octa_skeletonize(_native.ctx(m.device.index), ctypes.c_void_p(both.data_ptr()), 1, 65, 63, ctypes.c_void_p(both.data_ptr() + 100), None,
                              _native.current_stream_ptr())
    assert rc == -2
    rc = lib.octa_skeletonize(_native.ctx(m.device.index), p, 1, 0, 63, ctypes.c_void_p(both.data_ptr()), None, _native.current_stream_ptr())
    assert rc == -2
    torch.cuda.synchronize()
    assert torch.equal(m, before)


@pytest.fixture(scope="module")
def full_size_pair():
    """(label, perturbed copy) at 1216 x 1216 with their host skeletons and removing double passes; read-only."""
    from scipy.ndimage import binary_dilation
    g = np.load(os.path.join(GOLDEN, "raster_golden.npz"))
    label = np.unpackbits(np.asarray(g["graph0_label_packed"])).reshape(1216, 1216).astype(np.uint8)
    pred = (binary_dilation(label) & (np.random.default_rng(0).random(label.shape) >= 0.05)).astype(np.uint8)
    out = {"label": label, "pred": pred}
    for k in ("label", "pred"):
        out["skel_" + k], out["removing_" + k] = skeletonize_host(out[k], return_passes=True)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def test_full_size_pair_equals_host(full_size_pair, hip_lib_built):
    from octa_autosegmentation_amd.utils.metrics import ClDiceMetric
    f = full_size_pair
    assert int(f["skel_label"].sum()) == 166652 and f["removing_label"] + 1 == 16 and f["removing_pred"] + 1 == 24
    got, passes = _device(np.stack([f["label"], f["pred"]]))
    assert np.array_equal(got[0], f["skel_label"]) and np.array_equal(got[1], f["skel_pred"])
    assert passes == 24
    for k in ("label", "pred"):
        single, p = _device(np.array(f[k]))
        assert np.array_equal(single, f["skel_" + k]) and p == f["removing_" + k] + 1

    pred, label = torch.from_numpy(np.array(f["pred"]))[None].float(), torch.from_numpy(np.array(f["label"]))[None]
    host, dev = ClDiceMetric(), ClDiceMetric()
    host([pred], [label])
    dev([pred.cuda()], [label.cuda()])
    assert dev.scores[0].is_cuda and dev.scores[0].dim() == 0 and not host.scores[0].is_cuda
    print("clDice of the pair: host", float(host.scores[0]), "device", float(dev.scores[0]))
    assert abs(float(dev.scores[0]) - float(host.scores[0])) <= 1e-12
    assert abs(float(host.scores[0]) - 0.8899) <= 1e-3


def test_cldice_metric_on_the_device_matches_reference_scores(hip_lib_built):
    check_metric_against_golden("cuda")


def test_validate_cli_reports_cldice(tmp_path, hip_lib_built):
    """validate.py on configs/config_oof.yml (set up as tests/test_oof_gpu.py does): the result has Validation_ClDice in the reference's
    position, equal to the score computed on the host (skeletonize_host, numpy) from the same post-processed maps, rounded alike."""
    import validate as validate_cli
    from octa_autosegmentation_amd.data.image_dataset import get_dataset, get_post_transformation
    from octa_autosegmentation_amd.utils.config_overrides import apply_cli_overrides_from_unknown_args
    from octa_autosegmentation_amd.utils.enums import Phase
    from test_oof import CASES
    names = ["octa", "even"]
    images, labels = tmp_path / "images", tmp_path / "labels"
    images.mkdir()
    labels.mkdir()
    for i, name in enumerate(names):
        u8 = CASES[name]["u8"]
        Image.fromarray(u8).save(images / f"img_{i}.png")
        Image.fromarray(((u8 > 100) * 255).astype(np.uint8)).save(labels / f"img_{i}.png")
    split = tmp_path / "split.txt"
    split.write_text("".join(f"{i}\n" for i in range(len(names))))
    cfg_path = os.path.join(ROOT, "configs", "config_oof.yml")
    ov = ["--Validation.data.image.files", str(images / "*.png"), "--Validation.data.image.split", str(split),
          "--Validation.data.label.files", str(labels / "*.png"), "--Validation.data.label.split", str(split),
          "--General.device", "cuda:0", "--Output.save_dir", str(tmp_path / "out")]
    metrics = validate_cli.main(["--config_file", cfg_path, "--num_workers", "0"] + ov)
    assert list(metrics) == [f"Validation_{k}" for k in ("DSC", "IoU", "ClDice", "AUC", "ACC", "Recall", "Precision")]

    with open(cfg_path) as f:
        config = yaml.safe_load(f)
    apply_cli_overrides_from_unknown_args(config, ov)
    loader = get_dataset(config, Phase.VALIDATION, num_workers=0)
    post = get_post_transformation(config, Phase.VALIDATION)
    scores = []
    for i, batch in enumerate(loader):
        pred = post["prediction"](torch.from_numpy(CASES[names[i]]["out"]).cuda()[None])
        label = post["label"](batch["label"][0].to("cuda:0"))
        assert len(pred) == 1 and len(label) == 1
        v_p, v_l = pred[0].cpu().numpy().astype(np.float64), label[0].cpu().numpy().astype(np.float64)
        s_p, s_l = skeletonize_host(v_p), skeletonize_host(v_l)
        assert s_p.sum() > 0 and s_l.sum() > 0
        tprec, tsens = (v_p * s_l).sum() / s_l.sum(), (v_l * s_p).sum() / s_p.sum()
        scores.append(2 * tprec * tsens / (tprec + tsens))
    loader.close()
    expect = float(str(round(torch.tensor(np.nanmean(scores)).float().item(), 3)))        # Metric.aggregate hands a float32 on
    print("Validation_ClDice", metrics["Validation_ClDice"], "host", scores)
    assert np.isfinite(expect) and metrics["Validation_ClDice"] == expect
