"""CPU: the paper's noise-model augmentation on host tensors -- NoiseModeld against the reference's own outputs
(tests/golden/noise_model_golden.npz), RandomDecreaseResolutiond against the two torch interpolations it stands for, the registry on the
shipped RA config, and the counter-based generator of csrc/philox.h against the published known answers."""
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

import _noise_model_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
FACTORS = np.linspace(0.25, 1.0, 200).tolist()
SIZES = [(37, 53), (304, 304)]


def test_registry_builds_the_shipped_ra_config():
    from octa_autosegmentation_amd.data import data_transforms as T
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "config_ves_seg-S_RA.yml")))
    aug = cfg["Train"]["data_augmentation"]
    names = [d["name"] for d in aug]
    assert names.index("NoiseModeld") < names.index("Resized") < names.index("RandomDecreaseResolutiond")
    chain = dict(zip(names, T.get_data_augmentations(aug, seed=1)))
    nm, rd = chain["NoiseModeld"], chain["RandomDecreaseResolutiond"]
    assert isinstance(nm, T.NoiseModeld) and isinstance(rd, T.RandomDecreaseResolutiond)
    assert (nm.keys, nm.prob, nm.grid_size, nm.lambda_delta, nm.lambda_speckle, nm.lambda_gamma, nm.alpha, nm.downsample_factor) == \
        (["image"], 1, (9, 9), 1, 0.7, 0.3, 0.2, 1)
    assert (rd.keys, rd.p, rd.max_factor, rd.allow_missing_keys) == (["image"], 1, 0.25, True)
    assert nm.rng_streams() == {"python", "torch"} and rd.rng_streams() == {"python"}
    # both sides of NoiseModeld draw from python's `random`: the chain must not be cut into a batched form
    assert not T.Compose(list(chain.values())).batchable()
    for phase in ("Validation", "Test"):
        T.get_data_augmentations(cfg[phase]["data_augmentation"], seed=1)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_noise_model_on_cpu_tensors_is_the_reference_bit_for_bit(name):
    """Every recorded call of one instance: the output, where torch's generator stands afterwards, the untouched background. The second call
    of cases a and b only matches if the first call drew its control points twice."""
    g = C.golden()
    assert name in C.cases()
    res = C.run_case(name, CPU)
    assert len(res) == int(g[f"{name}_calls"])
    for c, (out, nxt, d) in enumerate(res):
        assert out.dtype == torch.float32 and not out.requires_grad
        assert np.array_equal(out.numpy(), g[f"{name}_{c}_out"])
        assert nxt == g[f"{name}_{c}_next"]
        assert np.array_equal(d["background"].numpy(), g[f"{name}_background"])


def test_noise_model_draws_one_python_random_and_skips_at_prob_zero():
    from octa_autosegmentation_amd.data import data_transforms as T
    g = C.golden()
    img, bg = torch.from_numpy(g["a_in"].copy()), torch.from_numpy(g["a_background"].copy())
    random.seed(5)
    torch.manual_seed(5)
    d = T.NoiseModeld(["image"], prob=0)({"image": img, "background": bg})
    after, t_after = random.random(), torch.rand(()).item()
    random.seed(5)
    torch.manual_seed(5)
    random.random()
    assert after == random.random() and t_after == torch.rand(()).item() and torch.equal(d["image"], img)
    with pytest.raises(KeyError):
        T.NoiseModeld(["image"])({"image": img})                      # no background: the reference's KeyError


def test_control_points_are_the_fixtures():
    """data/noise_model.py alone: the grids the device path would hand to the kernel are the ones the reference drew."""
    from octa_autosegmentation_amd.data.noise_model import NoiseModelDraws
    g = C.golden()
    torch.manual_seed(int(g["c_seed"]))
    grids = torch.cat(NoiseModelDraws((9, 9)).control_points(1), dim=1)[0]
    assert np.array_equal(grids.numpy(), g["c_0_grids"])
    raw = C.evaluate(*(torch.zeros(1, 40, 56),) * 2, torch.from_numpy(g["a_0_grids"])[None], *(torch.zeros(1, 40, 56),) * 2, (1, 0.7, 0.3), torch.float32)[2]
    assert np.array_equal(raw[0].numpy(), g["a_0_maps"]) and raw[0, :4].min().item() < 1e-3


def _two_interpolations(x, factor):
    d = F.interpolate(x.unsqueeze(0), scale_factor=factor)
    return F.interpolate(d, size=x.shape[1:]).squeeze(0)


@pytest.mark.parametrize("size", SIZES)
def test_decrease_resolution_equals_the_two_interpolations(size, monkeypatch):
    """200 factors evenly spaced in [0.25, 1]: the transform on CPU tensors, and the one-gather form with host-built index tables that CUDA
    tensors take, both equal interpolate(scale_factor) -> interpolate(size) exactly, with no exception."""
    from octa_autosegmentation_amd.data import data_transforms as T
    from octa_autosegmentation_amd.data.noise_model import nearest_roundtrip_tables
    x = torch.rand((1,) + size, generator=torch.Generator().manual_seed(size[0]))
    t = T.RandomDecreaseResolutiond(["image"])
    for f in FACTORS:
        want = _two_interpolations(x, f)
        draws = iter([0.0, f])
        monkeypatch.setattr(random, "uniform", lambda a, b: next(draws))
        got = t({"image": x})["image"]
        assert got.shape == x.shape and torch.equal(got, want), f
        rows, cols = nearest_roundtrip_tables(size, f)
        assert torch.equal(x.index_select(1, rows).index_select(2, cols), want), f


def test_decrease_resolution_draws_like_the_reference():
    """random.uniform(0, 1) < p, then one random.uniform(max_factor, 1) per key; nothing per key when the first draw refuses; a missing key
    raises although allow_missing_keys is set, as in the reference."""
    from octa_autosegmentation_amd.data import data_transforms as T
    x = torch.rand(1, 37, 53, generator=torch.Generator().manual_seed(0))
    for p, keys in ((1, ["image"]), (1, ["image", "label"]), (0, ["image"])):
        random.seed(11)
        d = T.RandomDecreaseResolutiond(keys, p=p, max_factor=0.25)({"image": x, "label": x})
        after = random.random()
        random.seed(11)
        want = {}
        if random.uniform(0, 1) < p:
            for k in keys:
                want[k] = _two_interpolations(x, random.uniform(0.25, 1))
        assert after == random.random()
        for k in ("image", "label"):
            assert torch.equal(d[k], want.get(k, x))
    with pytest.raises(KeyError):
        T.RandomDecreaseResolutiond(["image"])({"label": x})


def test_philox_known_answers(hip_lib_built):
    """Philox-4x32-10 of csrc/philox.h (the host build of the function the kernel calls) against the known-answer vectors published with the
    Random123 library: counter and key all zero, all ones, and the digits of pi."""
    from octa_autosegmentation_amd import _native
    kat = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for ctr, key, want in kat:
        c, k, o = np.array(ctr, np.uint32), np.array(key, np.uint32), np.zeros(4, np.uint32)
        _native.lib().octa_philox4x32_10(c.ctypes.data, k.ctypes.data, o.ctypes.data)
        assert o.tolist() == want
