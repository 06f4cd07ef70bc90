"""CPU: adversarial augmentation (models/noise_model_at.py AtLoss, Train.AT) -- the host restatement of the loop against recorded runs of the
reference's own ANTLoss / NoiseModel (tests/golden/noise_model_at_golden.npz, written by tools/make_golden_noise_model_at.py), the loss
registry, LambdaModel's binding and the shipped configs/config_ves_seg-S_AA.yml.

The reference's rotation is torchvision's, which is not installed where the fixture was made: the fixture was recorded with THIS package's
restatement (rotate_bilinear) injected into the reference, so it pins the loop around the rotation -- the order of the python-random and torch
draws, the label path, the three ascent steps on the control grids -- and not the rotation against torchvision."""
import ast
import functools
import os
import random
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "noise_model_at_golden.npz"))


def fixture_net(g, name):
    net = torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3, padding=1), torch.nn.LeakyReLU(0.01), torch.nn.Conv2d(4, 1, 3, padding=1))
    with torch.no_grad():
        for i, p in enumerate(net.parameters()):
            p.copy_(torch.from_numpy(g[f"{name}_net_{i}"].copy()))
    return net


@pytest.mark.parametrize("name", ["full", "crop"])
def test_host_loop_against_the_reference(name):
    """Same seeds, same network, same loss: the python-random draws in the reference's order, the label, the control grids as drawn (bit for
    bit: the first call's double draw included) and after each of the three ascent steps, and where both generators are left.
    The steps are float32 torch arithmetic in the reference's order, so on the CPU that wrote the fixture they are its bits; another CPU may
    order the convolutions' float32 sums differently, which moves a gradient by a few ulp of its largest terms: allowed is 1e-3 of the largest
    step of the iteration (a wrong sign, a missing grad_scale, a step on stale grids or a changed draw order are all of the order of a step)."""
    from octa_autosegmentation_amd.models.losses import DiceBCELoss, get_loss_function_by_name
    g = golden()
    kw = ast.literal_eval(str(g[f"{name}_at"]))
    x, bg, y = (torch.from_numpy(g[f"{name}_{k}"].copy()) for k in ("x", "background", "y"))
    net = fixture_net(g, name)
    torch.manual_seed(int(g[f"{name}_seed"]))
    # the fixture's python draws came from the global `random` after random.seed(seed); here they come from AtLoss's private stream under the
    # same seed (the same generator), and the global stream, which the device loader's thread advances in training, must stay untouched
    random.seed(12345)
    untouched = random.getstate()
    at = get_loss_function_by_name("AtLoss", {"Train": {"AT": kw or True}, "General": {}}, None, DiceBCELoss(True), seed=int(g[f"{name}_seed"]))
    assert at.grad_scale == 65536.0
    y_in = y.clone()
    adv, label = at(net, x, bg, y)
    assert torch.equal(y, y_in)                                                   # the caller's label is not thresholded in place
    assert np.array_equal(np.array(at.downsample_factor), g[f"{name}_downsample_factor"])
    assert np.array_equal(np.array(at.rot_k), g[f"{name}_rot_k"]) and np.array_equal(np.array(at.rot_r), g[f"{name}_rot_r"])
    if "crop" in kw:
        assert np.array_equal(np.array(at.h_crop), g[f"{name}_h_crop"]) and np.array_equal(np.array(at.w_crop), g[f"{name}_w_crop"])
    assert at.rng.random() == float(g[f"{name}_next_python"]) and random.getstate() == untouched
    assert np.float32(torch.rand(()).item()) == g[f"{name}_next_torch"]
    assert np.array_equal(label.numpy(), g[f"{name}_label"]) and set(np.unique(label.numpy())) <= {0.0, 1.0}
    want = g[f"{name}_grids"]
    got = np.stack([t.numpy() for t in at.grid_trajectory])
    assert got.shape == want.shape == (4, 2, 5, 9, 9)
    assert np.array_equal(got[0], want[0])
    for i in range(3):
        step = np.abs(want[i + 1] - want[i]).max()
        err = np.abs(got[i + 1] - want[i + 1]).max()
        print(f"[AT host loop, {name}] step {i + 1}: largest grid change {step:.3e}, deviation from the reference {err:.3e}", flush=True)
        assert step > 0 and err <= 1e-3 * step
    assert np.allclose(torch.stack(at.loss_trajectory).numpy(), g[f"{name}_losses"], rtol=1e-5, atol=0)
    assert adv.shape == label.shape and not adv.requires_grad and np.allclose(adv.numpy(), g[f"{name}_adv"], rtol=0, atol=1e-4)
    # the network is frozen inside the loop only, and the loop leaves it no gradient
    assert all(p.requires_grad and p.grad is None for p in net.parameters())


def test_second_call_redraws_the_grids_once_and_restores_frozen_flags():
    from octa_autosegmentation_amd.data.noise_model import NoiseModelDraws
    from octa_autosegmentation_amd.models.noise_model_at import AtLoss
    g = golden()
    x, bg, y = (torch.from_numpy(g[f"full_{k}"].copy()) for k in ("x", "background", "y"))
    net = fixture_net(g, "full")
    net[0].bias.requires_grad_(False)
    at = AtLoss(torch.nn.BCEWithLogitsLoss(), grad_scale=1.0)
    torch.manual_seed(5); random.seed(5)
    at(net, x, bg, y)
    first = at.grid_trajectory[0].clone()
    at(net, x, bg, y)
    assert [p.requires_grad for p in net.parameters()] == [True, False, True, True]
    # the draws alone, from the same seed: two sets at the first call, then the two Beta fields of each of the four samples, then one set
    torch.manual_seed(5)
    draws = NoiseModelDraws((9, 9))
    assert torch.equal(torch.cat(draws.control_points(2), dim=1), first)
    assert not torch.equal(at.grid_trajectory[0], first) and at.grid_trajectory[0].shape == first.shape


def test_rotation_restatement_geometry():
    """0 degrees is the identity, 90 degrees on a square image is rot90 counter-clockwise (torchvision's sense), a small angle keeps the centre."""
    from octa_autosegmentation_amd.models.noise_model_at import rotate_bilinear
    x = torch.rand(2, 1, 16, 16, generator=torch.Generator().manual_seed(0))
    assert torch.allclose(rotate_bilinear(x, 0.0), x, atol=1e-6)
    assert torch.allclose(rotate_bilinear(x, 90.0), torch.rot90(x, 1, dims=(-2, -1)), atol=1e-5)
    odd = torch.rand(1, 1, 15, 21, generator=torch.Generator().manual_seed(1))
    assert abs(rotate_bilinear(odd, 7.0)[0, 0, 7, 10].item() - odd[0, 0, 7, 10].item()) < 1e-6


def test_registry_and_lambda_model_accept_train_at():
    """Fails before this feature: the registry had no "AtLoss" and LambdaModel raised NotImplementedError for Train.AT."""
    from octa_autosegmentation_amd.models import networks
    from octa_autosegmentation_amd.models.lambda_model import LambdaModel
    from octa_autosegmentation_amd.models.losses import DiceBCELoss, get_loss_function_by_name
    from octa_autosegmentation_amd.models.noise_model_at import AtLoss
    from octa_autosegmentation_amd.utils.enums import Phase
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "config_ves_seg-S_AA.yml")))
    assert cfg["Train"]["AT"] == dict(grid_size=[9, 9], lambda_delta=1, lambda_speckle=0.7, lambda_gamma=0.3, max_decrease_res=0.25, alpha=0.001,
                                      grad_scale=65536.0)
    names = [t["name"] for t in cfg["Train"]["data_augmentation"]]
    assert "NoiseModeld" not in names and "Resized" not in names and "background" in cfg["Train"]["data_augmentation"][0]["keys"]
    loss = DiceBCELoss(True)
    at = get_loss_function_by_name("AtLoss", cfg, None, loss)
    assert isinstance(at, AtLoss) and at.loss_fun is loss and at.alpha == 0.001 and at.crop == (1, 1) and at.lambdas == (1, 0.7, 0.3)
    cfg["General"]["device"] = "cpu"
    cfg["Output"]["save_dir"] = os.path.join(ROOT, "results", "unused")
    model = LambdaModel(cfg["General"]["model"]["name"], Phase.TRAIN, networks.MODEL_DICT, **{k: v for k, v in cfg["General"]["model"].items() if k != "name"})
    model.initialize_model_and_optimizer(None, networks.init_weights, cfg, Namespace(start_epoch=0, epoch="latest"), None, Phase.TRAIN)
    assert isinstance(model.at, AtLoss) and model.at.grad_scale == 65536.0
    assert isinstance(model.at.rng, random.Random) and model.at.rng is not random          # a stream of its own, seeded from General.seed
    cfg["General"]["seed"] = 7
    a, b = (get_loss_function_by_name("AtLoss", cfg, None, loss).rng.random() for _ in range(2))
    cfg["General"]["seed"] = 8
    assert a == b != get_loss_function_by_name("AtLoss", cfg, None, loss).rng.random()
    plain = yaml.safe_load(open(os.path.join(ROOT, "configs", "config_ves_seg-S.yml")))
    plain["General"]["device"] = "cpu"
    other = LambdaModel("DynUNet", Phase.TRAIN, networks.MODEL_DICT, **{k: v for k, v in plain["General"]["model"].items() if k != "name"})
    other.initialize_model_and_optimizer(None, networks.init_weights, plain, Namespace(start_epoch=0, epoch="latest"), None, Phase.TRAIN)
    assert not hasattr(other, "at")
