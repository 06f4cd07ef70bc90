"""GPU parity of the augmentation kernels (csrc/augment.hip) against the torch ops MONAI's transforms delegate to:
F.interpolate(bilinear), torch.flip / torch.rot90, F.affine_grid + F.grid_sample. fp32, tolerance 1e-5 (same formulas,
fused multiply-adds may differ in the last bits).
The derived bounds now live in tests/_rotate_ref.py and tests/_speckle_ref.py (held by tests/test_rotate_gpu.py and tests/test_speckle_gpu.py);
this file keeps the torch-parity smoke checks and holds the whole chain to the composition of the float64 references."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHAIN_CONFIG = [{"name": "LoadGraphAndFilterByRandomRadiusd", "keys": ["image", "label"]},
                {"name": "ScaleIntensityd", "keys": ["image", "label"], "minv": 0, "maxv": 1},
                {"name": "EnsureChannelFirstd", "keys": ["image", "label"]},
                {"name": "Resized", "keys": ["image", "label"], "spatial_size": [128, 128], "mode": "bilinear"},
                {"name": "RandFlipd", "keys": ["image", "label"], "prob": 0.5, "spatial_axis": [0, 1]},
                {"name": "RandRotate90d", "keys": ["image", "label"], "prob": 0.75},
                {"name": "RandRotated", "keys": ["image", "label"], "prob": 1, "range_x": 0.1745, "padding_mode": "zeros"},
                {"name": "AsDiscreted", "keys": ["label"], "threshold": 0.1},
                {"name": "CastToTyped", "keys": ["image", "label"], "dtype": "dtype"}]


def test_resize_matches_torch_interpolate(hip_lib_built):
    import torch
    import torch.nn.functional as F
    from octa_autosegmentation_amd.data import gpu_augment
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randint(0, 256, (3, 76, 76), device="cuda", generator=g, dtype=torch.uint8)
    got = gpu_augment.resize_bilinear(x, [304, 304])
    want = F.interpolate(x.float().unsqueeze(1), size=(304, 304), mode="bilinear", align_corners=False).squeeze(1)
    assert (got - want).abs().max().item() <= 1e-3          # values up to 255
    xf = torch.rand(2, 50, 70, device="cuda", generator=g)
    mul, add = torch.tensor([2.0, 0.5], device="cuda"), torch.tensor([-1.0, 3.0], device="cuda")
    got = gpu_augment.resize_bilinear(xf, [125, 91], mul, add)
    want = F.interpolate((xf * mul[:, None, None] + add[:, None, None]).unsqueeze(1), size=(125, 91), mode="bilinear", align_corners=False).squeeze(1)
    assert (got - want).abs().max().item() <= 1e-5
    same = gpu_augment.resize_bilinear(xf, [50, 70])
    assert (same - xf).abs().max().item() <= 1e-6           # Resized to the same size is the identity


def test_resize_adjoint_matches_torch_autograd(hip_lib_built):
    """octa_resize_bilinear_bwd (round 4): the gradient of F.interpolate(bilinear) for the GAN-seg model's 304 -> 1216 up-sampling, a
    non-integer ratio, a down-sampling and the identity; through the autograd function on [B, C, h, w] in fp32 and bf16."""
    import torch
    import torch.nn.functional as F
    from octa_autosegmentation_amd.data import gpu_augment
    g = torch.Generator(device="cuda").manual_seed(4)
    for (h, w, H, W) in [(304, 304, 1216, 1216), (50, 70, 125, 91), (96, 64, 48, 40), (33, 17, 33, 17), (5, 3, 64, 64)]:
        x = torch.rand(2, 1, h, w, device="cuda", generator=g, requires_grad=True)
        dy = torch.randn(2, 1, H, W, device="cuda", generator=g)
        F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False).backward(dy)
        want = x.grad.clone()
        got = gpu_augment.resize_bilinear_bwd(dy.reshape(2, H, W).contiguous(), (h, w)).view(2, 1, h, w)
        assert (got - want).abs().max().item() <= 2e-5 * max(1.0, want.abs().max().item()), (h, w, H, W)
        x2 = x.detach().clone().requires_grad_(True)
        y2 = gpu_augment.BilinearResize.apply(x2, (H, W))
        assert (y2 - F.interpolate(x.detach(), size=(H, W), mode="bilinear", align_corners=False)).abs().max().item() <= 1e-5
        y2.backward(dy)
        assert (x2.grad - want).abs().max().item() <= 2e-5 * max(1.0, want.abs().max().item())
    xb = torch.rand(3, 2, 40, 40, device="cuda", generator=g).to(torch.bfloat16).requires_grad_(True)
    yb = gpu_augment.BilinearResize.apply(xb, (160, 160))
    assert yb.dtype == torch.bfloat16 and yb.shape == (3, 2, 160, 160)
    yb.float().sum().backward()
    assert xb.grad.dtype == torch.bfloat16 and abs(float(xb.grad.float().sum()) - 3 * 2 * 160 * 160) < 0.02 * 3 * 2 * 160 * 160      # the weights of every output pixel sum to one


def test_flip_rot90_rotate_matches_torch(hip_lib_built):
    import torch
    import torch.nn.functional as F
    from octa_autosegmentation_amd.data import gpu_augment
    g = torch.Generator(device="cuda").manual_seed(2)
    B, N = 8, 96
    x = torch.rand(B, N, N, device="cuda", generator=g)
    flip = torch.tensor([0, 1, 0, 1, 0, 1, 0, 1], dtype=torch.int32, device="cuda")
    k = torch.tensor([0, 0, 1, 1, 2, 2, 3, 3], dtype=torch.int32, device="cuda")
    ang = torch.tensor([0.0, 0.1, -0.17, 0.05, 0.17, -0.03, 0.12, -0.1], device="cuda")
    got = gpu_augment.flip_rot90_rotate(x, ang, k, flip)
    for b in range(B):
        y = x[b]
        if int(flip[b]):
            y = torch.flip(y, (0, 1))
        y = torch.rot90(y, int(k[b]), (0, 1))
        c, s = float(torch.cos(ang[b])), float(torch.sin(ang[b]))
        theta = torch.tensor([[[c, -s, 0.0], [s, c, 0.0]]], device="cuda")
        grid = F.affine_grid(theta, (1, 1, N, N), align_corners=False)
        want = F.grid_sample(y[None, None], grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0, 0]
        assert (got[b] - want).abs().max().item() <= 2e-5, b
    thr = gpu_augment.flip_rot90_rotate(x, ang, k, flip, threshold=0.5)
    assert set(thr.unique().tolist()) <= {0.0, 1.0}
    assert ((thr > 0.5) != (got >= 0.5)).float().mean().item() < 1e-4


def test_augmentation_chain_from_config(hip_lib_built):
    """The reference's config list drives the chain; image and label of a sample get the same geometry."""
    import torch
    from octa_autosegmentation_amd.data import gpu_augment
    cfg = CHAIN_CONFIG
    aug = gpu_augment.GpuSegAugmentation(cfg, seed=3)
    g = torch.Generator(device="cuda").manual_seed(4)
    img = torch.randint(0, 256, (6, 32, 32), device="cuda", generator=g, dtype=torch.uint8)
    lab = (torch.rand(6, 128, 128, device="cuda", generator=g) > 0.7).to(torch.uint8) * 255
    out = aug(img, lab)
    assert out["image"].shape == (6, 1, 128, 128) and out["label"].shape == (6, 1, 128, 128)
    assert out["image"].dtype == torch.float32 and 0.0 <= float(out["image"].min()) and float(out["image"].max()) <= 1.0 + 1e-6
    assert set(out["label"].unique().tolist()) <= {0.0, 1.0}
    p = out["params"]
    assert p["rot_k"].max() <= 3 and np.abs(p["angle"]).max() <= 0.1745 + 1e-6
    # same seed -> same decisions
    again = gpu_augment.GpuSegAugmentation(cfg, seed=3)(img, lab)
    assert torch.equal(again["image"], out["image"]) and torch.equal(again["label"], out["label"])


def _composition(x, size, params, win=None):
    """What the chain is configured to compute, in float64 on the inputs' device: ScaleIntensity(0, 1) with each image's own minimum and
    maximum (a constant image maps to minv), the bilinear resize of tests/_resize_ref.py, then the flip / rot90 / rotation of
    tests/_rotate_ref.py with the decisions the object reports. -> (reference before the threshold, tolerance): the rotate bound, with
    the resize bound carried through the rotation (the four weights sum to at most 1) and three roundings for the scale map, which the
    object forms in fp32 (1 / span, min * mul, minv - that)."""
    import torch
    import _resize_ref as rr
    import _rotate_ref as R
    xd = x.double()
    mn, mx = xd.amin((1, 2)), xd.amax((1, 2))
    span = mx - mn
    mul = torch.where(span > 0, 1.0 / span, torch.zeros_like(span))
    add = 0.0 - mn * mul
    y, tol_y = rr.forward(x, size[0], size[1], mul, add)
    scale = rr.U * (xd.abs().amax((1, 2)) * mul + 2.0 * mn.abs() * mul + add.abs())
    angle = torch.from_numpy(params["angle"]).to(x.device)
    return R.reference(y, angle, params["rot_k"], params["flip"], win=win, extra=tol_y.amax((1, 2)) + scale)


def _chain_inputs():
    """the batch of test_augmentation_chain_from_config with one constant image and one empty label in it (ScaleIntensity: mul = 0)"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(4)
    img = torch.randint(0, 256, (6, 32, 32), device="cuda", generator=g, dtype=torch.uint8)
    lab = (torch.rand(6, 128, 128, device="cuda", generator=g) > 0.7).to(torch.uint8) * 255
    img[2], lab[2] = 77, 0
    return img, lab


def _check_chain(out, img, lab, win=None):
    import torch
    import _rotate_ref as R
    p = out["params"]
    assert len(set(p["rot_k"].tolist())) > 1 and len(set(p["flip"].tolist())) == 2 and np.abs(p["angle"]).min() > 0
    ref, tol = _composition(img, (128, 128), p, win)
    rat = R.ratio(out["image"][:, 0], ref, tol)
    lref, ltol = _composition(lab, (128, 128), p, win)
    share = float((~R.decided(lref, ltol, 0.1)).sum((1, 2)).max()) / (lref.shape[1] * lref.shape[2])
    wrong, other = R.discrete(out["label"][:, 0], lref, ltol, 0.1)
    print("CHAIN", tuple(out["image"].shape), "image error / bound", float(f"{rat:.4g}"), "label: undecided share", share, "wrong", wrong, "not 0 or 1", other)
    assert rat <= 1.0
    assert share <= R.UNDECIDED_CAP and wrong == 0 and other == 0
    # the constant image is minv everywhere in front of the rotation, the empty label 0 behind the threshold: exactly
    assert bool((out["image"][2] == 0).all()) and bool((out["label"][2] == 0).all())
    assert float(out["label"].mean()) > 0.1 and float(out["image"].mean()) > 0.2


def test_augmentation_chain_is_the_configured_composition(hip_lib_built):
    """out["image"] and out["label"] ARE ScaleIntensity, Resized, flip, rot90 and rotation with the reported decisions, within the derived
    bounds; the label exactly on every decided pixel. Measured on an MI355X on the kernels of commit c9efa0d: image error / bound 0.060
    (0.041 in the 64 x 64 windows), 0.15 % of a label at most undecided, no decided pixel wrong."""
    from octa_autosegmentation_amd.data import gpu_augment
    img, lab = _chain_inputs()
    out = gpu_augment.GpuSegAugmentation(CHAIN_CONFIG, seed=3)(img, lab)
    assert out["image"].shape == out["label"].shape == (6, 1, 128, 128)
    _check_chain(out, img, lab)


@pytest.mark.parametrize("factor", [0.5, 1.25])
def test_augmentation_chain_with_the_crop_is_the_window_of_the_composition(hip_lib_built, factor):
    """with a RandCropOrPadd entry behind RandRotated: the reported window of that same composition (factor 1.25: the pad, negative offsets)"""
    from octa_autosegmentation_amd.data import gpu_augment
    cfg = CHAIN_CONFIG[:7] + [{"name": "RandCropOrPadd", "keys": ["image", "label"], "prob": 1, "min_factor": factor, "max_factor": factor}] + CHAIN_CONFIG[7:]
    img, lab = _chain_inputs()
    random.seed(7)
    out = gpu_augment.GpuSegAugmentation(cfg, seed=3)(img, lab)
    side = int(128 * factor)
    assert out["image"].shape == out["label"].shape == (6, 1, side, side)
    offs = list(zip(out["params"]["crop_oy"].tolist(), out["params"]["crop_ox"].tolist()))
    assert (len(set(offs)) > 1 and min(min(o) for o in offs) >= 0) if factor < 1 else offs == [(-16, -16)] * 6
    _check_chain(out, img, lab, ((side, side), offs))
    plain = gpu_augment.GpuSegAugmentation(CHAIN_CONFIG, seed=3)(img, lab)            # same seed, same decisions: the window of the full frame
    assert np.array_equal(plain["params"]["angle"], out["params"]["angle"]) and np.array_equal(plain["params"]["rot_k"], out["params"]["rot_k"])


def test_noise_kernels_match_the_reference_fixture(hip_lib_built):
    """a17 on the device: the HIP kernels behind SpeckleBrightnesd / AddRandomBackgroundNoised (csrc/augment.hip) against the outputs of
    the reference's own classes (tests/golden/noise_golden.npz, tools/make_golden_noise.py) with the same generator seeds. The
    background blend is exact (one float64 product, one comparison); the speckle map differs from torch's CPU arithmetic by fused
    multiply-adds only (1e-6 of values in [0, 1])."""
    import os
    import torch
    from octa_autosegmentation_amd.data import data_transforms as T
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "noise_golden.npz"))
    for k in range(2):
        img = torch.from_numpy(g[f"speckle_{k}_in"]).cuda()
        torch.manual_seed(100 + k)
        out = T.SpeckleBrightnesd(["image"])({"image": img.clone()})["image"]
        assert out.is_cuda and out.dtype == torch.float32
        assert (out.cpu() - torch.from_numpy(g[f"speckle_{k}_out"])).abs().max().item() <= 1e-6
        np.random.seed(200 + k)
        d = T.AddRandomBackgroundNoised(["image"])({"image": img.clone(), "background": torch.from_numpy(g[f"bg_{k}_noise"]).cuda()})
        assert d["image"].is_cuda and d["image"].dtype == torch.float64 and torch.equal(d["image"].cpu(), torch.from_numpy(g[f"bg_{k}_out"]))
    # batched entry points
    from octa_autosegmentation_amd.data import gpu_augment
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand(3, 64, 80, device="cuda", generator=gen)
    c9 = torch.rand(3, 9, 9, device="cuda", generator=gen) * 0.5 + 0.5
    u = torch.rand(3, 64, 80, device="cuda", generator=gen)
    got = gpu_augment.speckle_brightness(x, c9, u)
    C = torch.nn.functional.interpolate(c9[:, None], size=(64, 80), mode="bilinear")[:, 0]
    v = x * (C - u * (1 - C))
    want = v / v.amax(dim=(1, 2), keepdim=True)
    want = want - want.amin(dim=(1, 2), keepdim=True)
    assert (got - want).abs().max().item() <= 2e-6
    u64 = torch.rand(3, 64, 80, device="cuda", generator=gen, dtype=torch.float64)
    assert torch.equal(gpu_augment.background_noise(x, u, u64), torch.maximum(x.double(), u.double() * u64))
    assert torch.equal(gpu_augment.background_noise(x, u, u64, torch.float32), torch.maximum(x.double(), u.double() * u64).float())
