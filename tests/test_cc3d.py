"""CPU: the references of tests/_cc3d_ref.py agree with each other (scipy.ndimage.label + bincount against a breadth-first flood fill,
ties included), and the Python layer of the 3-D connected-component filter is registered: transforms, arguments, the native symbol."""
import ctypes
import os

import numpy as np
import pytest

import _cc3d_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("connectivity", [1, 2, 3])
def test_scipy_restatement_equals_the_flood_fill(connectivity):
    rng = np.random.default_rng(40 + connectivity)
    shapes = [(5, 7, 9), (1, 7, 9), (5, 1, 9), (4, 6, 1), (2, 2, 2), (3, 5, 9)]
    for i in range(12):
        shape = shapes[i % len(shapes)]
        m = (rng.random(shape) < (0.15, 0.3, 0.45, 0.6)[i % 4]).astype(np.uint8)
        assert np.array_equal(ref.keep_largest(m, connectivity), ref.flood_keep_largest(m, connectivity)), (shape, i)
    # ties: isolated voxels only (every component has one voxel, the first in C order wins), and the two bars
    m = np.zeros((5, 7, 9), np.uint8)
    m[::2, ::2, ::2] = 1
    want = np.zeros_like(m)
    want[0, 0, 0] = 1
    assert np.array_equal(ref.keep_largest(m, connectivity), want) and np.array_equal(ref.flood_keep_largest(m, connectivity), want)
    bars = ref.two_bars()
    want = np.zeros_like(bars)
    want[0, 0, :3] = 1
    assert np.array_equal(ref.keep_largest(bars, connectivity), want) and np.array_equal(ref.flood_keep_largest(bars, connectivity), want)
    assert ref.info(bars, connectivity) == (2, 3, 0)
    assert ref.info(np.zeros((2, 3, 4), np.uint8), connectivity) == (0, 0, -1)


def test_pinned_volumes_and_fixtures():
    vols = ref.pinned_volumes()
    for shape, want in ref.PINNED.items():
        assert ref.info(vols[shape], 3)[:2] == want
    lab, _ = ref.label(vols[(9, 70, 67)], 3)
    assert np.sort(np.bincount(lab.ravel())[1:])[-2] == 14
    s = ref.serpentine()
    assert ref.info(s, 1) == (1, int(s.sum()), 0)
    assert all(s[z:z + 4, y:y + 8, x:x + 64].any() for z in range(0, 12, 4) for y in range(0, 40, 8) for x in range(0, 200, 64))


def test_remove_outer_noise_restatement():
    """Specks above and below the slab go, whatever is connected to the central plane stays; the filled plane itself is not added."""
    v = np.zeros((9, 12, 12), np.float32)
    v[4, 2:10, 3] = 1          # in the central plane
    v[5, 9, 4] = 1             # touches it diagonally (26-neighbourhood)
    v[6:8, 9, 5] = 1           # and on from there
    v[0, 0:4, 0:4] = 1         # a 16-voxel speck far above: larger than anything else, but not connected to the plane
    out = ref.remove_outer_noise(v)
    want = v.astype(bool)
    want[0] = False
    assert out.dtype == np.bool_ and np.array_equal(out, want)
    with pytest.raises(IndexError):
        ref.remove_outer_noise(np.zeros((9, 70, 67), np.float32), z_axis=1)


def test_transforms_are_registered():
    from octa_autosegmentation_amd.data import data_transforms as dt
    assert "RemoveOuterNoise" in dt.TRANSFORMS and "KeepLargestConnectedComponent" in dt.TRANSFORMS


def test_get_data_augmentations_builds_them():
    from octa_autosegmentation_amd.data import data_transforms as dt
    augs = dt.get_data_augmentations([{"name": "RemoveOuterNoise", "z_axis": 0}, {"name": "KeepLargestConnectedComponent"},
                                      {"name": "RemoveSmallObjects", "min_size": 16, "independent_channels": False}])
    assert isinstance(augs[0], dt.RemoveOuterNoise) and augs[0].z_axis == 0
    assert isinstance(augs[1], dt.KeepLargestConnectedComponent) and augs[1].connectivity is None
    assert augs[2].independent_channels is False and dt.RemoveSmallObjects().independent_channels is True


@pytest.mark.parametrize("kwargs, named", [({"applied_labels": [1]}, "applied_labels"), ({"is_onehot": True}, "is_onehot"),
                                           ({"independent": False}, "independent"), ({"num_components": 2}, "num_components")])
def test_keep_largest_rejects_what_is_not_built(kwargs, named):
    from octa_autosegmentation_amd.data import data_transforms as dt
    with pytest.raises(NotImplementedError, match=named):
        dt.KeepLargestConnectedComponent(**kwargs)


def test_cpu_tensors_raise():
    import torch
    from octa_autosegmentation_amd.data import data_transforms as dt
    x = torch.zeros(1, 4, 5, 6)
    for t in (dt.RemoveOuterNoise(), dt.KeepLargestConnectedComponent(), dt.RemoveSmallObjects(independent_channels=False)):
        with pytest.raises(RuntimeError, match="GPU"):
            t(x[0] if isinstance(t, dt.RemoveOuterNoise) else x)


def test_native_symbol_signature():
    from octa_autosegmentation_amd import _native
    c_int, c_void_p = ctypes.c_int, ctypes.c_void_p
    assert _native.SIGNATURES["octa_cc3d_filter"] == (c_int, [c_void_p, c_void_p] + [c_int] * 7 + [ctypes.c_uint8, c_void_p, c_void_p, c_void_p])
    header = open(os.path.join(ROOT, "include", "octa_hip.h")).read()
    assert "int octa_cc3d_filter(octa_ctx *ctx, const uint8_t *d_in, int B, int D, int H, int W, int connectivity, int mode, int min_size," in header


def test_entry_point_rejects_bad_arguments(hip_lib_built):
    """Every -2 of the entry point is decided before the context or a buffer is touched: no GPU needed (the addresses are never read)."""
    from octa_autosegmentation_amd import _native
    l = _native.lib()
    assert l.octa_abi_version() == 2
    ctx, d_in, d_out = 4096, 1 << 32, 1 << 40
    ok = dict(ctx=ctx, d_in=d_in, B=1, D=4, H=5, W=6, connectivity=3, mode=1, min_size=0, on_value=1, d_out=d_out, d_info=None, stream=None)
    for change, word in (({"ctx": None}, "bad pointers"), ({"d_in": None}, "bad pointers"), ({"d_out": None}, "bad pointers"),
                         ({"d_out": d_in + 7}, "bad pointers"), ({"B": 0}, "positive"), ({"D": -1}, "positive"), ({"H": 0}, "positive"),
                         ({"W": 0}, "positive"), ({"connectivity": 0}, "connectivity"), ({"connectivity": 4}, "connectivity"),
                         ({"mode": 2}, "mode"), ({"mode": -1}, "mode"), ({"D": 2048, "H": 1024, "W": 1024}, "2^31"),
                         ({"B": 3, "D": 1024, "H": 1024, "W": 1024}, "2^31")):
        assert l.octa_cc3d_filter(*{**ok, **change}.values()) == -2, change
        assert word in l.octa_last_error().decode(), (change, l.octa_last_error().decode())


def test_config_carries_the_commented_entry():
    text = open(os.path.join(ROOT, "configs", "config_3d_recon_supervised.yml")).read()
    assert text.count("# - name: RemoveOuterNoise") == 2
    import yaml
    cfg = yaml.safe_load(text)
    for phase in ("Train", "Test"):
        assert [d["name"] for d in cfg[phase]["post_processing"]["prediction"]] == ["Activations", "AsDiscrete", "RemoveSmallObjects", "AsChannelLast"]
