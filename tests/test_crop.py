"""CPU: RandCropOrPadd (the Giarratano set-up's random crop) on host tensors against the reference's own outputs
(tests/golden/crop_golden.npz), the registry, its declared random stream, and which chains the fused batch loader accepts."""
import copy
import os
import random

import numpy as np
import pytest
import torch
import yaml

import _crop_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _chain(name):
    return yaml.safe_load(open(os.path.join(ROOT, "configs", name)))["Train"]["data_augmentation"]


@pytest.mark.parametrize("name", C.CASES)
def test_rand_crop_or_pad_on_cpu_tensors_is_the_reference_bit_for_bit(name):
    shapes = C.check_case(name, "cpu")
    if name == "prob":
        assert len(shapes) == 2              # applied and not applied calls
    if name == "range":
        assert len(shapes) == 3              # one factor per call


def test_pad_case_floors_an_odd_difference_and_returns_float32():
    g = C.golden()
    out = g["pad_u8_out0_image"]
    assert g["pad_u8_in_image"].dtype == np.uint8 and out.dtype == np.float32 and out.shape == (1, 31, 40)
    # (31 - 24) // 2 = 3 rows and (40 - 31) // 2 = 4 columns of zeros in front, one more behind
    assert np.array_equal(out[:, 3:27, 4:35], g["pad_u8_in_image"].astype(np.float32))
    assert out[:, :3].max() == 0 and out[:, 27:].max() == 0 and out[:, :, :4].max() == 0 and out[:, :, 35:].max() == 0


def test_giarratano_sizes_shapes_offsets_and_stream():
    """[1, 1216, 1216] with 0.2965: 360 x 360 windows at the reference's offsets (rows drawn first), stream position afterwards."""
    from octa_autosegmentation_amd.data import data_transforms as T
    assert int(1216 * 0.2965) == 360
    g = C.golden()
    prob, lo, hi = g["big_args"].tolist()
    t = T.RandCropOrPadd(["image", "label"], prob=prob, min_factor=lo, max_factor=hi)
    ramp = torch.arange(1216 * 1216, dtype=torch.float32).reshape(1, 1216, 1216)
    random.seed(int(g["big_seed"]))
    for shape, (oy, ox) in zip(g["big_shapes"].tolist(), g["big_offsets"].tolist()):
        d = t({"image": ramp, "label": ramp})
        assert list(d["image"].shape) == shape == [1, 360, 360] and t.offsets == (oy, ox)
        assert torch.equal(d["image"], ramp[:, oy:oy + 360, ox:ox + 360]) and torch.equal(d["label"], d["image"])
    assert random.random() == float(g["big_after"])


def test_later_keys_take_the_first_keys_slices():
    from octa_autosegmentation_amd.data import data_transforms as T
    t = T.RandCropOrPadd(["image", "label"], prob=1, min_factor=0.5, max_factor=0.5)
    random.seed(3)
    a, b = torch.rand(1, 20, 30), torch.rand(2, 40, 60)
    d = t({"image": a, "label": b, "other": 7})
    oy, ox = t.offsets
    assert torch.equal(d["image"], a[:, oy:oy + 10, ox:ox + 15]) and torch.equal(d["label"], b[:, oy:oy + 10, ox:ox + 15]) and d["other"] == 7


def test_registry_knows_rand_crop_or_pad():
    from octa_autosegmentation_amd.data import data_transforms as T
    (t,) = T.get_data_augmentations([{"name": "RandCropOrPadd", "keys": ["image", "label"], "prob": 1, "min_factor": 0.2965, "max_factor": 0.2965}], seed=1)
    assert isinstance(t, T.RandCropOrPadd) and (t.keys, t.prob, t.min_factor, t.max_factor) == (["image", "label"], 1, 0.2965, 0.2965)
    d = T.RandCropOrPadd(["image"])
    assert (d.prob, d.min_factor, d.max_factor) == (0.1, 1, 1)
    for phase in ("Train", "Validation", "Test"):          # the shipped config builds
        cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "config_ves_seg-S_Giarratano.yml")))
        T.get_data_augmentations(cfg[phase]["data_augmentation"], seed=1)


def test_missing_key_raises_key_error():
    from octa_autosegmentation_amd.data import data_transforms as T
    with pytest.raises(KeyError):
        T.RandCropOrPadd(["image", "label"], prob=1, min_factor=0.5, max_factor=0.5)({"image": torch.zeros(1, 8, 8)})


def test_chain_with_the_crop_behind_a_batched_transform_is_not_batchable():
    """The S_GAN Giarratano chain: graph loader (global `random`) ... ImageToImageTranslationd (batch form) ... RandCropOrPadd (global
    `random`): cutting it at the batched transform would reorder the draws, so Compose refuses."""
    from octa_autosegmentation_amd.data import data_transforms as T

    class Translation:
        def __call__(self, data):
            return data

        def batch_apply(self, samples):
            return samples

    load = T.LoadGraphAndFilterByRandomRadiusd(["image", "label"], image_resolutions=[[304, 304], [1216, 1216]], min_radius=[0, 0])
    crop = T.RandCropOrPadd(["image", "label"], prob=1, min_factor=0.2965, max_factor=0.2965)
    assert crop.rng_streams() == {"python"}
    assert not T.Compose([load, Translation(), crop]).batchable()
    assert T.Compose([load, Translation(), T.AsDiscreted(["label"], threshold=0.1)]).batchable()       # the crop is what forbids the cut


def test_fused_loader_accepts_the_giarratano_chain_only_when_every_sample_gets_one_window(monkeypatch):
    from octa_autosegmentation_amd.data.image_dataset import FusedGraphSegBatches
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    chain = _chain("config_ves_seg-S_Giarratano.yml")
    at = [d["name"] for d in chain].index("RandCropOrPadd")
    assert [d["name"] for d in chain][at - 1:at + 2] == ["RandRotated", "RandCropOrPadd", "AsDiscreted"]
    assert FusedGraphSegBatches.applies(chain)
    assert FusedGraphSegBatches.applies(_chain("config_ves_seg-S.yml"))

    def variant(**kw):
        c = copy.deepcopy(chain)
        c[at].update(kw)
        return c

    assert not FusedGraphSegBatches.applies(variant(prob=0.5))
    assert not FusedGraphSegBatches.applies(variant(min_factor=0.2, max_factor=0.2965))
    assert not FusedGraphSegBatches.applies(variant(keys=["image"]))
    moved = copy.deepcopy(chain)
    moved.insert(at + 1, moved.pop(at))                      # behind AsDiscreted: not the accepted place
    assert not FusedGraphSegBatches.applies(moved)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert not FusedGraphSegBatches.applies(chain)
