"""tools/make_golden_frangi.py -- generates tests/golden/frangi_golden.npz, frangi_golden_mask.npz and frangi_golden_304.npz: the
reference's models/frangi.py (its calling convention: x255, sigmas (0.5, 2, 0.5), alpha 1, beta 15, bright ridges, float64
output, the view) on a stand-in for the absent scikit-image -- tools/frangi_scipy.py, skimage >= 0.25's algorithm restated over
scipy.ndimage, registered as `skimage.filters.frangi`. Parity with scikit-image itself is not pinned.

Runs ONLY in the build container: imports /root/reference/models/frangi.py at run time (nothing of it is committed). The five
inputs of the OOF fixtures (tests/test_oof.py CASES: odd 91 x 97, even 64 x 48, octa 304^2, crop 400^2 mask, full 1216^2 mask) are
reused, not stored again; six tiny uint8 inputs are added (img = u8.astype(float32) / float32(div)):
  t1x1, t1x25, t25x1 (lines shorter than every radius), const (5 x 7, all 9), rand57 (5 x 7 random: reflects several times at
  R = 35), checker (8 x 9 checkerboard of 0 / 255: exact eigenvalue ties). The reference squeezes the image, which would drop an
  axis of length 1: for the three one-pixel-wide inputs the stand-in is called directly, with the reference's arguments.
Per case: `<case>_gamma` (float32), `<case>_out` (float64, every `<case>_outstep`-th pixel of both axes) and per scale k (0: sigma
0.5, 1: sigma 2; the third repeats the first and is asserted identical) the Hessian planes and sorted eigenvalues
`<case>_s<k>_{hrr,hrc,hcc,l1,l2}` (float32, every `<case>_step`-th pixel) with `<case>_s<k>_sha`: SHA-256 of each FULL plane's bytes
after `+ 0.0` (signed zeros are not part of the contract), in that order. For crop and full, `<case>_tie_idx` (scale, row, column)
lists every pixel whose eigenvalues tie in magnitude with opposite signs, with `_tie_l1`, `_tie_l2` and the final `_tie_out`
there; full also has the exact max, min and sum of the output. `w_s<k>_o<order>` are scipy's own `_gaussian_kernel1d` tables.

Asserted here, for the cases the end-to-end tests use: no output within 2^-17 of the configuration's thresholds (octa: 0.04 and
0.75; even: 0.04) and at least one object left after RemoveSmallObjects. Re-running rewrites the three files byte for byte."""
import hashlib
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch
from scipy import ndimage as ndi
from scipy.ndimage._filters import _gaussian_kernel1d

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF = "/root/reference"
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import frangi_scipy  # noqa: E402

TRACE = []
PLANES = ("hrr", "hrc", "hcc", "l1", "l2")


def standin_frangi(image, **kwargs):
    assert image.dtype == np.float32 and image.ndim == 2, (image.dtype, image.shape)
    assert kwargs == dict(sigmas=(0.5, 2, 0.5), alpha=1, beta=15, black_ridges=False), kwargs
    return frangi_scipy.frangi(image, trace=TRACE, **kwargs)


def reference_frangi():
    sk, flt = types.ModuleType("skimage"), types.ModuleType("skimage.filters")
    flt.frangi = standin_frangi
    sk.filters = flt
    sys.modules["skimage"], sys.modules["skimage.filters"] = sk, flt
    spec = importlib.util.spec_from_file_location("reference_frangi", os.path.join(REF, "models", "frangi.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Frangi


def sha(plane):
    return hashlib.sha256(np.ascontiguousarray(plane + np.float32(0.0)).tobytes()).hexdigest()


def case(Frangi, name, img, step, outstep, ties=False):
    del TRACE[:]
    t = torch.from_numpy(np.ascontiguousarray(img))[None, None]
    if 1 in img.shape:      # the reference's squeeze() would drop the axis: the same call on the 2-D array
        out = torch.tensor(standin_frangi(t[0, 0].numpy() * 255, sigmas=(0.5, 2, 0.5), alpha=1, beta=15, black_ridges=False)).view(t.shape)
    else:
        out = Frangi()(t)
    assert out.dtype == torch.float64 and out.shape == t.shape
    out = out.numpy()[0, 0]
    assert len(TRACE) == 3
    for k in PLANES:
        assert TRACE[0][k].dtype == np.float32 and TRACE[0][k].tobytes() == TRACE[2][k].tobytes()
    d = {f"{name}_step": np.int64(step), f"{name}_outstep": np.int64(outstep), f"{name}_gamma": np.float32(TRACE[0]["gamma"]),
         f"{name}_out": out[::outstep, ::outstep].copy()}
    tie_idx, tie_l1, tie_l2 = [], [], []
    for s in (0, 1):
        tr = TRACE[s]
        d[f"{name}_s{s}_sha"] = np.array([sha(tr[k]) for k in PLANES], dtype="S64")
        for k in PLANES:
            d[f"{name}_s{s}_{k}"] = tr[k][::step, ::step].copy()
        yy, xx = np.nonzero((tr["l1"] == -tr["l2"]) & (tr["l1"] != 0))
        for y, x in zip(yy, xx):
            tie_idx.append((s, y, x))
            tie_l1.append(tr["l1"][y, x])
            tie_l2.append(tr["l2"][y, x])
    if ties:
        idx = np.array(tie_idx, dtype=np.int32).reshape(-1, 3)
        d.update({f"{name}_tie_idx": idx, f"{name}_tie_l1": np.array(tie_l1, np.float32), f"{name}_tie_l2": np.array(tie_l2, np.float32),
                  f"{name}_tie_out": out[idx[:, 1], idx[:, 2]].copy()})
    print(f"{name}: {img.shape} gamma {float(d[f'{name}_gamma'])!r} ties {len(tie_idx)} out max {out.max():.6f}")
    return d, out


def check_threshold(name, out, threshold, min_size):
    margin = np.abs(out - threshold).min()
    lab, n = ndi.label(out > threshold)        # connectivity 1, as RemoveSmallObjects
    kept = int((np.bincount(lab.ravel())[1:] >= min_size).sum())
    print(f"  {name} at {threshold}: margin {margin:.3g}, {kept} of {n} objects kept (min_size {min_size})")
    assert margin > 2.0 ** -17 and kept >= 1, (name, threshold, margin, kept)


def write_npz(path, arrays):
    """numpy's .npz layout with fixed member dates, so that the bytes depend on the contents only."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    size = os.path.getsize(path)
    print(os.path.basename(path), size, "bytes")
    assert size < (1 << 20)


def main():
    from test_oof import CASES
    from octa_autosegmentation_amd.models.frangi import scaled_sigma_and_radius
    Frangi = reference_frangi()
    rng = np.random.default_rng(20261018)
    checker = ((np.add.outer(np.arange(8), np.arange(9)) % 2) * 255).astype(np.uint8)
    tiny = {"t1x1": np.array([[200]], np.uint8), "t1x25": rng.integers(0, 256, (1, 25), dtype=np.uint8),
            "t25x1": rng.integers(0, 256, (25, 1), dtype=np.uint8), "const": np.full((5, 7), 9, np.uint8),
            "rand57": rng.integers(0, 256, (5, 7), dtype=np.uint8), "checker": checker}

    small = {}
    for s, sigma in enumerate((0.5, 2)):
        sp, radius = scaled_sigma_and_radius(sigma)
        for order in (0, 1):
            small[f"w_s{s}_o{order}"] = _gaussian_kernel1d(sp, order, radius)
    for name, u8 in tiny.items():
        d, out = case(Frangi, name, u8.astype(np.float32) / np.float32(255), 1, 1)
        small.update(d)
        small[f"{name}_u8"], small[f"{name}_div"] = u8, np.float32(255)
        if name in ("t1x1", "const"):
            assert not out.any()
    for name in ("odd", "even"):
        d, out = case(Frangi, name, CASES[name]["img"], 1, 1)
        small.update(d)
        if name == "even":
            check_threshold(name, out, 0.04, 5)
    small["names"] = np.array(sorted(tiny) + ["odd", "even"], dtype="S16")
    write_npz(os.path.join(GOLDEN, "frangi_golden.npz"), small)

    mask = {}
    d, out = case(Frangi, "crop", CASES["crop"]["img"], 4, 4, ties=True)
    mask.update(d)
    d, out = case(Frangi, "full", CASES["full"]["img"], 16, 8, ties=True)
    mask.update(d, full_out_max=np.float64(out.max()), full_out_min=np.float64(out.min()), full_out_sum=np.float64(out.sum()))
    mask["names"] = np.array(["crop", "full"], dtype="S16")
    write_npz(os.path.join(GOLDEN, "frangi_golden_mask.npz"), mask)

    d, out = case(Frangi, "octa", CASES["octa"]["img"], 8, 1)
    check_threshold("octa", out, 0.04, 5)
    check_threshold("octa", out, 0.75, 31)
    d["names"] = np.array(["octa"], dtype="S16")
    write_npz(os.path.join(GOLDEN, "frangi_golden_304.npz"), d)


if __name__ == "__main__":
    main()
