"""CPU: the host side of the 3-D reconstruction set-up (configs/config_3d_recon_supervised.yml): SelectSlice, AsChannelLast, NIfTI / npy
volumes through LoadImaged, and the shipped config."""
import os

import numpy as np
import torch
import yaml

from octa_autosegmentation_amd import nifti
from octa_autosegmentation_amd.data import data_transforms as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _volume(shape=(6, 5, 13)):
    return np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape)


def test_select_slice_against_hand_written_slicing():
    t = torch.from_numpy(_volume((13, 4, 5)))
    d = {"label": t, "image": torch.zeros(1, 4, 5)}
    out = T.SelectSlice(["label"], slice_selection=[[5, -4]])(d)
    assert out["label"].shape == (4, 4, 5) and torch.equal(out["label"], t[5:9]) and out["image"] is d["image"]
    out = T.SelectSlice(["label"], slice_selection=[[1, 12], [0, 3]])(d)
    assert torch.equal(out["label"], t[1:12, 0:3])
    assert T.SelectSlice(["label"], slice_selection=None)(d)["label"] is t
    assert T.SelectSlice(["label"])(d)["label"] is t
    assert "label" not in T.SelectSlice(["label"], allow_missing_keys=True, slice_selection=[[0, 1]])({"image": t})
    try:
        T.SelectSlice(["label"], slice_selection=[[0, 1]])({"image": t})
    except KeyError:
        pass
    else:
        raise AssertionError("a missing key must raise unless allow_missing_keys")


def test_as_channel_last_against_hand_written_permutation():
    t = torch.from_numpy(_volume((4, 6, 5)))
    assert torch.equal(T.AsChannelLast()(t), t.permute(1, 2, 0))
    assert torch.equal(T.AsChannelLast(channel_dim=0)(t), t.permute(1, 2, 0))
    assert torch.equal(T.AsChannelLast(channel_dim=1)(t), t.permute(0, 2, 1))


def test_both_are_built_from_yaml_dicts():
    text = """
    - name: SelectSlice
      keys:
      - label
      slice_selection: [[5,-4]]
    - name: AsChannelLast
      channel_dim: 0
    """
    sel, last = T.get_data_augmentations(yaml.safe_load(text))
    assert isinstance(sel, T.SelectSlice) and sel.slice_selection == (slice(5, -4),) and sel.keys == ["label"]
    assert isinstance(last, T.AsChannelLast) and last.channel_dim == 0


def test_volumes_keep_their_axis_order_through_the_loader(tmp_path):
    vol = _volume((6, 5, 13))                                        # [X, Y, Z]
    nii, npy = str(tmp_path / "v_3d_label.nii.gz"), str(tmp_path / "v.npy")
    nifti.write(nii, vol)
    np.save(npy, vol)
    chain = T.Compose(T.get_data_augmentations([
        dict(name="LoadImaged", keys=["label"], image_only=True),
        dict(name="EnsureChannelFirstd", keys=["label"], strict_check=False, channel_dim=2),
        dict(name="SelectSlice", keys=["label"], slice_selection=[[5, -4]])]))
    for path in (nii, npy):
        loaded = T.LoadImaged(["label"])({"label": path})["label"]
        assert loaded.dtype == torch.float32 and torch.equal(loaded.cpu(), torch.from_numpy(vol))           # no axis swap
        out = chain({"label": path})["label"].cpu()
        assert out.shape == (13 - 9, 6, 5) and torch.equal(out, torch.from_numpy(vol).permute(2, 0, 1)[5:9])


def test_shipped_config_parses_and_its_transform_lists_build():
    with open(os.path.join(ROOT, "configs", "config_3d_recon_supervised.yml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["General"]["model"]["out_channels"] == 44 and cfg["General"]["amp"] is True and cfg["Train"]["loss"] == "DiceBCELoss"
    names = {}
    for phase in ("Train", "Test"):
        augs = T.get_data_augmentations(cfg[phase]["data_augmentation"], seed=1, dtype=torch.bfloat16)
        names[phase] = [type(a).__name__ for a in augs]
        for chain in cfg[phase]["post_processing"].values():
            assert type(T.get_data_augmentations(chain)[-1]).__name__ == "AsChannelLast"
    assert names["Train"][:2] == ["LoadImaged", "LoadGraphAndFilterByRandomRadiusd"] and "SelectSlice" in names["Train"]
    sel = [d for d in cfg["Train"]["data_augmentation"] if d["name"] == "SelectSlice"][0]
    assert sel["slice_selection"] == [[5, -4]] and sel["keys"] == ["label"]
