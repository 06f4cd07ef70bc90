"""CPU: the sketch-filter baseline's host side (models/skrgan.py), the definition of the area opening its kernel follows
(tests/_morph_ref.py: the brute-force definition, the union-find restatement and the kernel's seed formulation agree), and the
whole filter restated over numpy against the fixture (tests/golden/skrgan_golden.npz, tools/make_golden_skrgan.py: the reference's
models/skrgan.py on a stand-in for scikit-image). Every comparison is exact: the opening performs no arithmetic and every other
stage has a fixed rounding order. tests/test_skrgan_gpu.py holds the kernels to the same references."""
import hashlib
import os

import numpy as np
import pytest
import torch

from octa_autosegmentation_amd.models import skrgan as skr_mod

from _morph_ref import brute_opening, closing, seed_opening, uf_opening
from test_frangi import np_pass
from test_oof import CASES as OOF_CASES, GOLDEN, ROOT

PLANES = ("mag", "filt", "open", "out")
LAMBDAS = (1, 2, 5, 17, 63, 64, 65, 128)
TINY = ["r8x8", "r9x8", "r12x11", "r20x23", "steps"]
NAN_FROM = {"r8x8": 2, "r9x8": 3, "r12x11": 3}        # the first plane of PLANES that is NaN everywhere (a constant stage before it)


def load_cases():
    z = np.load(os.path.join(GOLDEN, "skrgan_golden.npz"))
    cases = {}
    for name in (n.decode() for n in z["names"]):
        c = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}
        c["img"] = OOF_CASES[name]["img"] if name in OOF_CASES else c["u8"].astype(np.float32) / np.float32(255)
        cases[name] = c
    return cases, z["w_sigma2"]


CASES, SCIPY_TABLE = load_cases()


def canon(plane):
    """signed zeros and the sign and payload of a NaN are not part of the contract"""
    return np.where(np.isnan(plane), np.float32(np.nan), plane + np.float32(0.0))


def sha(plane):
    return hashlib.sha256(np.ascontiguousarray(canon(plane)).tobytes()).hexdigest().encode()


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(canon(a), canon(b), equal_nan=True)


def normalise(x):
    with np.errstate(invalid="ignore"):
        x = x - x.min()
        return x / x.max()


def np_sketch(img, sigma=2, area_open=64, area_close=64):
    """(mag, filt, open, out) of one float32 image: numpy, np_pass (tests/test_frangi.py) and the union-find opening."""
    diff, smooth = np.array([1.0, 0.0, -1.0]), np.array([1.0, 2.0, 1.0])        # correlate [-1, 0, 1] and [1, 2, 1], as np_pass takes them
    sh = np_pass(np_pass(img, 0, diff, 1), 1, smooth, 0)
    sv = np_pass(np_pass(img, 1, diff, 1), 0, smooth, 0)
    mag = normalise(np.sqrt(sh * sh + sv * sv))
    w = skr_mod.gaussian_weights(sigma)
    filt = mag if w is None else np_pass(np_pass(mag, 0, w, 0), 1, w, 0)
    if np.isnan(filt).any():
        return mag, filt, filt, filt
    opened = normalise(uf_opening(filt, area_open))
    if np.isnan(opened).any():
        return mag, filt, opened, opened
    out = normalise(closing(opened, area_close))
    assert all(p.dtype == np.float32 for p in (mag, filt, opened, out))
    return mag, filt, opened, out


def quantised(rng, shape, levels):
    return (rng.integers(0, levels, shape) / np.float32(levels - 1)).astype(np.float32)


def plateau_plane(rng, shape):
    """random blocks of 2 x 3 pixels of equal value: plateaus next to each other"""
    h, w = shape
    small = rng.random(((h + 1) // 2, (w + 2) // 3)).astype(np.float32)
    return np.ascontiguousarray(np.repeat(np.repeat(small, 2, axis=0), 3, axis=1)[:h, :w])


def definition_planes():
    rng = np.random.default_rng(11)
    planes = []
    for i in range(12):
        shape = tuple(int(v) for v in rng.integers(1, 21, 2))
        planes += [rng.random(shape).astype(np.float32), quantised(rng, shape, 3), quantised(rng, shape, 6), plateau_plane(rng, shape)]
    planes += [rng.random((20, 20)).astype(np.float32), quantised(rng, (20, 20), 3), np.full((9, 9), np.float32(0.25))]
    return planes


def test_definition_union_find_and_seed_formulation_agree():
    n = 0
    for f in definition_planes():
        for lam in LAMBDAS:
            if f.size < lam:
                continue
            ref = brute_opening(f, lam)
            assert np.array_equal(uf_opening(f, lam), ref), (f.shape, lam)
            if f.size <= 150 and lam <= 65:         # the growth per seed is slow in Python
                assert np.array_equal(seed_opening(f, lam), ref), (f.shape, lam)
            assert np.isin(ref, f).all() and (ref <= f).all()
            n += 1
    assert n > 150
    f = np.float32([[0, 5, 0, 3, 0]])
    assert np.array_equal(brute_opening(f, 1), f) and np.array_equal(brute_opening(f, 2), np.zeros_like(f))
    assert np.array_equal(closing(np.float32([[1, 0.25, 1, 0.5, 1]]), 2), np.ones((1, 5), np.float32))


def test_weight_table_constant_runtime_and_scipy_agree_bit_for_bit():
    assert skr_mod.gaussian_radius(2) == 8 and skr_mod.gaussian_radius(0.5) == 2 and skr_mod.gaussian_radius(5) == 20
    const, built = skr_mod.gaussian_weights(2), skr_mod._build_weights(2)
    assert const.dtype == np.float64 and const.shape == (17,)
    assert const.tobytes() == SCIPY_TABLE.tobytes() and built.tobytes() == SCIPY_TABLE.tobytes()
    assert skr_mod.gaussian_weights(0) is None and skr_mod.gaussian_weights(1e-16) is None
    w = skr_mod.gaussian_weights(3)
    assert w.shape == (25,) and np.array_equal(w, w[::-1]) and abs(w.sum() - 1) < 1e-15


@pytest.mark.parametrize("name", TINY + ["even", "odd"])
def test_numpy_restatement_reproduces_fixture(name):
    c = CASES[name]
    st = int(c["step"])
    got = np_sketch(c["img"])
    for i, (k, plane) in enumerate(zip(PLANES, got)):
        assert plane.dtype == np.float32
        full = k == "out" and c[k].shape == plane.shape
        assert same(plane if full else plane[::st, ::st], c[k]), (name, k)
        assert sha(plane) == c["sha"][i], (name, k)
        assert np.isnan(plane).all() == (name in NAN_FROM and i >= NAN_FROM[name]) and np.isnan(plane).all() == np.isnan(plane).any()


def test_fixture_holds_what_the_gpu_tests_need():
    assert sorted(CASES) == sorted(TINY + ["odd", "even", "crop", "full", "octa"])
    assert CASES["octa"]["out"].shape == (304, 304) and CASES["even"]["out"].shape == (64, 48)
    for c in CASES.values():
        assert all(c[k].dtype == np.float32 for k in PLANES) and c["sha"].shape == (4,)
    for name in ("odd", "even", "octa", "crop", "full"):
        assert not any(np.isnan(CASES[name][k]).any() for k in PLANES)
    for name in ("even", "octa"):              # stored in full: a normalised plane
        assert CASES[name]["out"].min() == 0 and CASES[name]["out"].max() == 1


def test_constructor_defaults_and_the_ignored_threshold_quirk(monkeypatch):
    f = skr_mod.SkrGAN()
    assert (f.sigma, f.area_threshold_open, f.connectivity_open, f.area_threshold_close, f.connectivity_close) == (2, 64, 1, 64, 1)
    assert f.eval() is f and f.train() is f
    g = skr_mod.SkrGAN(3, 5, 2, 7, 2)
    assert (g.sigma, g.area_threshold_open, g.connectivity_open, g.area_threshold_close, g.connectivity_close) == (3, 5, 2, 7, 2)
    seen = []
    monkeypatch.setattr(skr_mod, "sketch_filter", lambda img, *a: seen.append(a) or img)
    x = torch.zeros(1, 1, 8, 8)
    assert g(x) is x and seen == [(3, 64, 64)]             # sigma is honoured, the stored thresholds and connectivities are not


def test_refusals():
    x = torch.zeros(1, 1, 8, 8)
    for call in (lambda: skr_mod.area_opening(x), lambda: skr_mod.area_closing(x), lambda: skr_mod.sketch_filter(x), lambda: skr_mod.SkrGAN()(x)):
        with pytest.raises(RuntimeError, match="--General.device cuda:0"):
            call()
    small = torch.zeros(1, 1, 7, 9)
    for call in (lambda: skr_mod.area_opening(small), lambda: skr_mod.area_closing(small, 64), lambda: skr_mod.SkrGAN()(small),
                 lambda: skr_mod.sketch_filter(torch.zeros(8, 9), area_close=73)):
        with pytest.raises(ValueError, match="fewer than the area threshold"):
            call()
    for call in (lambda: skr_mod.area_opening(x, 64, connectivity=2), lambda: skr_mod.area_closing(x, 64, 2)):
        with pytest.raises(ValueError, match="connectivity"):
            call()
    for bad in (0, 129, 2.5):
        with pytest.raises(ValueError, match="area threshold"):
            skr_mod.area_opening(torch.zeros(20, 20), bad)


def test_wrong_dtype_is_refused(monkeypatch):
    monkeypatch.setattr(skr_mod, "_require_cuda", lambda t, who: None)     # the dtype check sits behind the device check
    for call in (lambda t: skr_mod.area_opening(t), lambda t: skr_mod.area_closing(t), lambda t: skr_mod.SkrGAN()(t)):
        for dt in (torch.float64, torch.float16, torch.uint8):
            with pytest.raises(TypeError, match="float32"):
                call(torch.zeros(1, 1, 8, 8, dtype=dt))


def test_define_model_gives_lambda_model_around_skrgan():
    import yaml
    from octa_autosegmentation_amd.models.lambda_model import LambdaModel
    from octa_autosegmentation_amd.models.model import define_model
    from octa_autosegmentation_amd.models.networks import MODEL_DICT
    from octa_autosegmentation_amd.utils.enums import Phase
    assert MODEL_DICT["skrgan"] is skr_mod.SkrGAN
    with open(os.path.join(ROOT, "configs", "config_skrgan.yml")) as f:
        config = yaml.safe_load(f)
    assert config["General"]["device"] == "cuda:0" and config["General"]["model"]["name"] == "skrgan"
    for ph in ("Validation", "Test"):
        assert config[ph]["post_processing"]["prediction"][0] == {"name": "AsDiscrete", "threshold": 0.5}
    config["General"]["device"] = "cpu"        # construction only
    model = define_model(config, phase=Phase.VALIDATION)
    assert isinstance(model, LambdaModel) and isinstance(model.model, skr_mod.SkrGAN) and model.model.sigma == 2
    model.initialize_model_and_optimizer(None, None, config, None, None, phase=Phase.VALIDATION)
    assert model.loss_function is None
    config["General"]["model"] = {"name": "skrgan", "sigma": 3, "area_threshold_open": 68}      # the reference's search driver sets these
    model = define_model(config, phase=Phase.VALIDATION)
    assert model.model.sigma == 3 and model.model.area_threshold_open == 68


def test_entry_points_validate_their_arguments_before_any_launch(hip_lib_built):
    """Shapes, thresholds, pixel counts, tables and pointers are refused with -2 on the host: no GPU is touched (the device pointers are fake)."""
    from octa_autosegmentation_amd import _native
    l = _native.lib()
    ws_bytes = l.octa_skr_workspace_bytes
    assert ws_bytes(1, 4097, 8) == 0 and ws_bytes(1, 8, 0) == 0 and ws_bytes(0, 8, 8) == 0 and ws_bytes(65536, 8, 8) == 0
    assert ws_bytes(2, 5, 7) >= 6 * 2 * 5 * 7 * 4 + 3 * 2 * 3 * 4
    a, b = 256, 4096
    opening = lambda h, w, lam, closing=0, ws=None, src=a, dst=b: l.octa_area_opening(src, dst, 1, h, w, lam, closing, ws, None)
    assert opening(0, 8, 64) == -2 and b"1 <= h, w <= 4096" in l.octa_last_error()
    for lam in (0, 129, -1):
        assert opening(20, 20, lam) == -2 and b"area threshold" in l.octa_last_error()
    assert opening(7, 9, 64) == -2 and b"at least that many pixels" in l.octa_last_error()
    assert opening(8, 8, 64, closing=1) == -2 and b"null pointer" in l.octa_last_error()
    assert opening(8, 8, 64, dst=None) == -2 and b"null pointer" in l.octa_last_error()
    assert opening(8, 8, 64, dst=a) == -2 and b"must not be the input" in l.octa_last_error()
    w = skr_mod.gaussian_weights(2)
    filt = lambda h, wd, radius, wt, ao, ac, ws=a, out=b: l.octa_skr_filter(a, None, None, None, out, 1, h, wd, radius, wt, ao, ac, ws, None)
    assert filt(8, 4097, 8, w.ctypes.data, 64, 64) == -2
    assert filt(8, 8, 8, w.ctypes.data, 65, 64) == -2 and b"at least that many pixels" in l.octa_last_error()
    assert filt(8, 8, 8, w.ctypes.data, 64, 129) == -2 and b"area threshold" in l.octa_last_error()
    assert filt(8, 8, 8, None, 64, 64) == -2 and b"weight table" in l.octa_last_error()
    assert filt(8, 8, 8, w.ctypes.data, 64, 64, ws=None) == -2 and b"null pointer" in l.octa_last_error()
    big = skr_mod.gaussian_weights(40)                      # 160 taps per side, none of them zero
    assert len(big) == 321
    assert filt(8, 8, 160, big.ctypes.data, 64, 64) == -2 and b"non-zero taps" in l.octa_last_error()
