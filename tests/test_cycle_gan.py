"""CPU: the CycleGAN baseline (models/cycle_gan.py, models/gan_loss.py) against the reference-made fixture
tests/golden/cyclegan_golden.npz (tools/make_golden_cyclegan.py), the host restatements of the csrc/gan_loss.hip kernels against
autograd, and train.py / test.py on a four-sample directory."""
import os
import random
import sys
from argparse import Namespace
from copy import deepcopy

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import make_golden_cyclegan as mk  # noqa: E402


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "cyclegan_golden.npz"))


def build_model(lambda_idt, pool_size, device="cpu", amp=False, phase=None, inference=None):
    from octa_autosegmentation_amd.models import networks
    from octa_autosegmentation_amd.models.model import define_model
    from octa_autosegmentation_amd.utils.enums import Phase
    phase = phase or Phase.TRAIN
    config = {"General": {"device": device, "amp": amp, "inference": inference, "model": mk.model_config(lambda_idt, pool_size)},
              "Train": dict(mk.TRAIN), "Output": {"save_dir": "/tmp"}}
    model = define_model(deepcopy(config), phase)
    if phase == Phase.TRAIN:
        model.initialize_model_and_optimizer(None, networks.init_weights, config, Namespace(start_epoch=0, epoch="latest"), None, Phase.TRAIN)
        for name in mk.NETS:
            mk.he_weights(getattr(model, name), mk.SALTS[name])
        model._after_weight_surgery()
        model.train()
    return model


def run_fixture_variant(tag, device="cpu", amp=False):
    """The four steps of one fixture variant on this repository's CycleGAN -> (losses, gradient norms, checksums, stream positions)."""
    lambda_idt, pool_size, background = mk.VARIANTS[tag]
    model = build_model(lambda_idt, pool_size, device, amp)
    torch.manual_seed(mk.TORCH_SEED)
    random.seed(int(golden()[f"{tag}_random_seed"]))
    return mk.run(model, background, device=device)


@pytest.mark.parametrize("tag", list(mk.VARIANTS))
def test_cycle_gan_update_matches_the_reference_fixture(tag):
    """Four consecutive updates against the reference's own CycleGAN.perform_training_step: step-1 losses depend on the forward
    composition alone (which generator sees which input, the background draws), the later ones on both optimisers' updates and on
    the image pools; the gradient norms pin the backward composition (frozen discriminators in the G pass, detached and pooled fakes in the
    D passes), the stream positions the number and order of the draws from `random` and torch's generator. Tolerances: those of the
    GAN-seg fixture (tests/test_models.py) -- the same torch on the same machine, a different batching of identical per-sample work."""
    threads = torch.get_num_threads()
    torch.set_num_threads(min(threads, 8))            # the later steps amplify rounding: the host's core count must not pick the reduction order
    try:
        losses, gnorm, sums, stream = run_fixture_variant(tag)
    finally:
        torch.set_num_threads(threads)
    g = golden()
    for step in range(mk.STEPS):
        print(f"[cyclegan {tag}] step {step + 1} max rel dev: losses {np.max(np.abs(losses[step] - g[f'{tag}_losses'][step]) / np.abs(g[f'{tag}_losses'][step])):.2e}, "
              f"grad norms {np.max(np.abs(gnorm[step] - g[f'{tag}_grad_norms'][step]) / g[f'{tag}_grad_norms'][step]):.2e}", flush=True)
    for step in range(mk.STEPS):
        assert np.allclose(losses[step], g[f"{tag}_losses"][step], rtol=2e-5 if step == 0 else 1e-3, atol=0), (step, losses[step], g[f"{tag}_losses"][step])
    assert np.allclose(gnorm, g[f"{tag}_grad_norms"], rtol=2e-3, atol=0), (gnorm, g[f"{tag}_grad_norms"])
    # the second column (sum of magnitudes) is the well-conditioned checksum; the plain sums cancel to ~1e-5 of it, hence their slack
    assert np.allclose(sums[:, 1], g[f"{tag}_param_sums"][:, 1], rtol=1e-6, atol=0), (sums, g[f"{tag}_param_sums"])
    assert np.allclose(sums[:, 0], g[f"{tag}_param_sums"][:, 0], rtol=1e-6, atol=0.5), (sums, g[f"{tag}_param_sums"])
    assert tuple(stream) == tuple(g[f"{tag}_stream"]), (stream, g[f"{tag}_stream"])
    assert g[f"{tag}_losses"][0][1] > 1.0            # and a sign error would not pass: the adversarial terms enter loss_G with a plus sign


@pytest.mark.parametrize("tag", ["bg", "idt05"])
def test_batched_passes_give_the_first_step_of_the_fixture(tag, monkeypatch):
    """The device form of the step -- three generator sequences and two discriminator sequences over concatenated batches -- forced on
    the CPU: the first step (no optimiser update behind it) within the fixture's first-step tolerances. The later steps are held
    by the unbatched CPU run above; batched, three Adam steps amplify the other summation order to 1e-2 in the gradient norms."""
    from octa_autosegmentation_amd.models import cycle_gan
    monkeypatch.setattr(cycle_gan, "USE_BATCHED_PASSES", True)
    lambda_idt, pool_size, background = mk.VARIANTS[tag]
    model = build_model(lambda_idt, pool_size)
    calls = []
    for name in mk.NETS:
        getattr(model, name).register_forward_hook(lambda mod, inp, out, name=name: calls.append((name, inp[0].shape[0])))
    torch.manual_seed(mk.TORCH_SEED)
    random.seed(int(golden()[f"{tag}_random_seed"]))
    _, l = model.perform_training_step(mk.batch(background), None, None, "cpu")
    assert calls == [("netG_A", 4), ("netG_B", 6), ("netG_A", 2), ("netD_A", 2), ("netD_B", 2), ("netD_A", 4), ("netD_B", 4)]
    g = golden()
    assert np.allclose([float(l[k]) for k in mk.LOSS_KEYS], g[f"{tag}_losses"][0], rtol=2e-5, atol=0)
    assert np.allclose(mk.grad_norms(model), g[f"{tag}_grad_norms"][0], rtol=2e-3, atol=0)


def test_image_pool_replays_the_recorded_sequence():
    """The reference's ImagePool alone: 40 queries of three constant planes carrying serial numbers, at a seed where batches draw one
    slot twice (the second image must receive the first, the slot keep the second). Returned serials, final pool and stream position."""
    from octa_autosegmentation_amd.models.cycle_gan import ImagePool
    g = golden()
    random.seed(int(g["pool_random_seed"]))
    pool = ImagePool(mk.POOL_SIZE)
    got, pos = mk.run_pool(pool)
    first = np.arange(1, mk.POOL_QUERIES * mk.POOL_BATCH + 1).reshape(mk.POOL_QUERIES, mk.POOL_BATCH)[:, :1]
    assert ((g["pool_returned"] >= first) & (g["pool_returned"] != first + np.arange(mk.POOL_BATCH))).any()       # the fixture holds the hard case
    assert (got == g["pool_returned"]).all(), (got, g["pool_returned"])
    assert (pool.images[:, 0, 0, 0].numpy().astype(np.int64) == g["pool_final"]).all() and pool.images.shape == (mk.POOL_SIZE, 1, 2, 2)
    assert pos == float(g["pool_stream"])
    # pool_size 0 hands the input through and draws nothing
    random.seed(1)
    x = torch.rand(2, 1, 2, 2)
    assert ImagePool(0).query(x) is x
    random.seed(1)
    assert random.random() == random.Random(1).random()


def _tied(shape, seed):
    """float64 values on a coarse grid: many exact ties between two such tensors."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 4, shape, generator=g).double() / 4


def test_l1_restatement_against_autograd():
    from octa_autosegmentation_amd.models import gan_loss
    preds = [_tied((2, 1, 5, 7), 1).requires_grad_(True), _tied((3, 1, 4, 4), 2).requires_grad_(True), _tied((7,), 3).requires_grad_(True)]
    targets = [_tied((2, 1, 5, 7), 4), _tied((3, 1, 4, 4), 5), _tied((7,), 3)]            # the last pair is equal everywhere
    ws = (10.0, 0.5, 3.0)
    assert all(((p == t).any() and (p != t).any()) for p, t in zip(preds[:2], targets[:2]))
    want_terms = [w * torch.nn.functional.l1_loss(p, t) for p, t, w in zip(preds, targets, ws)]
    want = sum(want_terms)
    g = torch.tensor(0.75, dtype=torch.float64)
    (want * g).backward()
    sums = gan_loss.l1_pairs_sums_host(preds, targets)
    out = gan_loss.l1_pairs_finish_host(sums, [p.numel() for p in preds], ws)
    assert out.dtype == torch.float32 and torch.allclose(out[:3].double(), torch.stack(want_terms).detach(), rtol=1e-6) and abs(float(out[3]) - float(want.detach())) <= 1e-6 * float(want.detach())
    got = gan_loss.l1_pairs_bwd_host(g, [p.detach() for p in preds], targets, ws)
    for d, p, t in zip(got, preds, targets):
        assert d.dtype == p.dtype and torch.allclose(d, p.grad, rtol=1e-6, atol=0)
        assert (d[p.detach() == t] == 0).all()                                      # sign(0) = 0
    assert (got[2] == 0).all()
    # the autograd function on CPU tensors is the restatement
    ps = [p.detach().float().requires_grad_(True) for p in preds]
    total, terms = gan_loss.l1_pairs([(p, t.float(), w) for p, t, w in zip(ps, targets, ws)])
    assert not terms.requires_grad and torch.equal(terms, out[:3]) and torch.equal(total.detach(), out[3])
    (total * 0.75).backward()
    for p, q in zip(ps, preds):
        assert torch.allclose(p.grad.double(), q.grad, rtol=1e-6, atol=0)


def test_lsgan_restatement_against_autograd():
    from octa_autosegmentation_amd.models import gan_loss
    ps = [torch.rand(2, 1, 2, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(1)).requires_grad_(True),
          torch.rand(3, 1, 14, 14, dtype=torch.float64, generator=torch.Generator().manual_seed(2)).requires_grad_(True)]
    targets, scales = (1.0, 0.0), (0.5, 0.5)
    want_terms = [s * ((p - t) ** 2).mean() for p, t, s in zip(ps, targets, scales)]
    g = torch.tensor(1.25, dtype=torch.float64)
    (sum(want_terms) * g).backward()
    sums, loss = gan_loss.lsgan_host(ps, targets, scales)
    assert torch.allclose(loss[:2].double(), torch.stack(want_terms).detach(), rtol=1e-6) and abs(float(loss[2]) - float(sum(want_terms))) <= 1e-6
    for d, p in zip(gan_loss.lsgan_bwd_host(g, [p.detach() for p in ps], targets, scales), ps):
        assert torch.allclose(d, p.grad, rtol=1e-6, atol=1e-12)
    qs = [p.detach().float().requires_grad_(True) for p in ps]
    total, terms = gan_loss.lsgan([(qs[0], True, 0.5), (qs[1], False, 0.5)])
    assert torch.equal(total.detach(), loss[2]) and torch.equal(terms, loss[:2])
    (total * 1.25).backward()
    for q, p in zip(qs, ps):
        assert torch.allclose(q.grad.double(), p.grad, rtol=1e-5, atol=1e-9)


def test_mix_max_restatement_against_autograd():
    from octa_autosegmentation_amd.models import gan_loss
    x = _tied((2, 1, 6, 6), 7)
    x[0, 0, :2] = 0                                    # the empty background of a rasterised graph against an empty background tile
    bg, u = _tied((2, 1, 6, 6), 8), _tied((2, 1, 6, 6), 9)
    bg[0, 0, :2] = 0
    x.requires_grad_(True)
    m = bg * u
    assert (x == m).sum() > 12 and (x > m).any() and (x < m).any()
    dout = torch.rand(2, 1, 6, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    torch.maximum(x, m).backward(dout)
    assert torch.equal(gan_loss.mix_max_host(x.detach(), bg, u), torch.maximum(x.detach(), m))
    got = gan_loss.mix_max_bwd_host(x.detach(), bg, u, dout)
    assert torch.allclose(got, x.grad, rtol=1e-6, atol=0)            # the restatement passes through float32
    tie = x.detach() == m
    assert torch.allclose(got[tie], 0.5 * dout[tie], rtol=1e-6) and (got[x.detach() < m] == 0).all()
    xf = x.detach().float().requires_grad_(True)
    gan_loss.mix_max(xf, bg.float(), u.float()).backward(dout.float())
    assert torch.allclose(xf.grad.double(), x.grad, rtol=1e-6, atol=0)


def test_registry_and_small_cases():
    from octa_autosegmentation_amd.models import losses, networks
    from octa_autosegmentation_amd.models.cycle_gan import CycleGAN
    from octa_autosegmentation_amd.utils.enums import Phase
    assert networks.MODEL_DICT["CycleGAN"] is CycleGAN
    assert isinstance(losses.get_loss_function_by_name("L1Loss"), torch.nn.L1Loss) and isinstance(losses.get_loss_function_by_name("LSGANLoss"), losses.LSGANLoss)
    # inference: only the named generator exists
    m = build_model(1.0, 2, phase=Phase.TEST, inference="netG_B")
    assert m.netG_A is None and m.netD_A is None and m.netD_B is None and isinstance(m.netG_B, networks.ResnetGenerator)
    assert [n for n, _ in m.named_children()] == ["netG_B"]
    m = build_model(1.0, 2, phase=Phase.TEST, inference="netG_A")
    assert m.netG_B is None and isinstance(m.netG_A, networks.ResnetGenerator)
    # lambda_idt = 0: runs, reports zeros, skips the identity passes
    model = build_model(0.0, 2)
    calls = []
    for name in ("netG_A", "netG_B"):
        getattr(model, name).register_forward_hook(lambda mod, inp, out, name=name: calls.append((name, inp[0].shape[0])))
    torch.manual_seed(0)
    random.seed(0)
    out, l = model.perform_training_step(mk.batch(True), None, None, "cpu")
    assert list(l) == list(mk.LOSS_KEYS) and float(l["idt_A"]) == 0 and float(l["idt_B"]) == 0 and out["idt_A"] is None
    assert all(np.isfinite(float(v)) for v in l.values()) and float(l["cycle_A"]) > 0
    assert calls == [("netG_A", 2), ("netG_B", 2), ("netG_B", 2), ("netG_A", 2)]                # no identity passes
    assert out["prediction"][0].shape == (1, 32, 32) and out["fake_B"].shape == (1, 1, 32, 32) and out["real_B_seg"].shape == (1, 1, 32, 32)
    model = build_model(1.0, 2)
    out, l = model.perform_training_step(mk.batch(False), None, None, "cpu")
    assert out["idt_A"].shape == (1, 1, 32, 32)
    assert abs(float(l["G"]) - sum(float(l[k]) for k in ("G_A", "G_B", "cycle_A", "cycle_B", "idt_A", "idt_B"))) <= 1e-5 * float(l["G"])
    # another criterion is an error, not a silent change of the objective
    from octa_autosegmentation_amd.models.model import define_model
    cfg = {"General": {"device": "cpu", "amp": False, "model": mk.model_config(1.0, 2)}, "Train": dict(mk.TRAIN, loss_criterionCycle="MSELoss"),
           "Output": {"save_dir": "/tmp"}}
    with pytest.raises(NotImplementedError):
        define_model(deepcopy(cfg), Phase.TRAIN).initialize_model_and_optimizer(None, networks.init_weights, cfg, Namespace(start_epoch=0, epoch="latest"), None, Phase.TRAIN)


def png_dataset(root, n=4, size=32):
    """Four synthetic-looking, four real-looking and four background PNGs."""
    from PIL import Image
    rng = np.random.default_rng(0)
    for sub in ("synthetic", "real", "background"):
        os.makedirs(os.path.join(root, sub))
    for i in range(n):
        a = np.zeros((size, size), np.uint8)
        for _ in range(3):
            r, c = rng.integers(3, size - 3, 2)
            a[r - 1:r + 1, :] = 255; a[:, c:c + 1] = 200
        Image.fromarray(a).save(os.path.join(root, "synthetic", f"a{i}.png"))
        Image.fromarray(np.clip(a * 0.5 + rng.normal(50, 15, a.shape), 0, 255).astype(np.uint8)).save(os.path.join(root, "real", f"b{i}.png"))
        Image.fromarray(rng.integers(0, 80, (size, size)).astype(np.uint8)).save(os.path.join(root, "background", f"g{i}.png"))


def cli_config(root, out, device="cpu", amp=False):
    keys = ["real_A", "real_B", "background"]
    load = lambda ks, missing: [dict({"name": "LoadImaged", "keys": ks, "image_only": True}, **missing), dict({"name": "ToGrayScaled", "keys": ks}, **missing),
                                dict({"name": "ScaleIntensityd", "keys": ks, "minv": 0, "maxv": 1}, **missing),
                                dict({"name": "EnsureChannelFirstd", "keys": ks, "strict_check": False, "channel_dim": "no_channel"}, **missing)]
    files = lambda sub: {"files": os.path.join(root, sub, "*.png")}
    nets = mk.model_config(1.0, 3)
    return {"General": {"amp": amp, "device": device, "task": "gan-ves-seg", "inference": "netG_A", "seed": 5, "model": nets},
            "Train": {"data": {"real_A": files("synthetic"), "real_B": files("real"), "background": files("background")},
                      "epochs": 1, "epochs_decay": 0, "save_interval": 1, "batch_size": 2, "lr": 2e-4,
                      "loss_criterionGAN": "LSGANLoss", "loss_criterionCycle": "L1Loss", "loss_criterionIdt": "L1Loss",
                      "data_augmentation": load(keys, {}) + [{"name": "RandFlipd", "keys": ["real_A"], "prob": 0.5, "spatial_axis": [0, 1]},
                                                             {"name": "RandFlipd", "keys": ["real_B", "background"], "prob": 0.5, "spatial_axis": [0, 1]},
                                                             {"name": "CastToTyped", "keys": keys, "dtype": "dtype"}],
                      "post_processing": {"prediction": [{"name": "AsDiscrete", "threshold": 0.5}], "label": [{"name": "AsDiscrete", "threshold": 0.5}]}},
            "Test": {"batch_size": 1, "data": {"real_A": files("synthetic"), "background": files("background")}, "save_comparisons": False,
                     "data_augmentation": load(["real_A", "background"], {"allow_missing_keys": True}) + [
                         {"name": "AddRandomBackgroundNoised", "keys": ["real_A"]},
                         {"name": "CastToTyped", "keys": ["real_A"], "allow_missing_keys": True, "dtype": "dtype"}],
                     "post_processing": {"prediction": None, "label": None}},
            "Output": {"save_dir": out, "save_to_disk": True, "save_to_tensorboard": False}}


def check_cli_run(run, written, size):
    """What train.py and test.py leave behind for a CycleGAN run."""
    from PIL import Image
    rows = open(os.path.join(run, "metrics.csv")).read().splitlines()
    assert rows[0] == "epoch," + ",".join(f"train_{k}" for k in mk.LOSS_KEYS) + ",Train_DSC,Train_IoU" and len(rows) == 2
    assert np.isfinite([float(v) for v in rows[1].split(",")]).all()
    names = set(os.listdir(os.path.join(run, "checkpoints")))
    assert {f"latest_{n}_model.pth" for n in mk.NETS + ("optimizer_G", "optimizer_D")} <= names
    ck = torch.load(os.path.join(run, "checkpoints", "latest_netG_A_model.pth"), weights_only=False)
    assert set(ck) == {"epoch", "model", "optimizer", "config"} and ck["epoch"] == 1 and "model.1.weight" in ck["model"]
    ck = torch.load(os.path.join(run, "checkpoints", "latest_optimizer_D_model.pth"), weights_only=False)
    assert ck["optimizer"]["param_groups"][0]["betas"] == (0.5, 0.999)
    assert any(n.startswith("sample_train_latest") for n in os.listdir(run))
    assert len(written) == 4 and all(os.path.basename(w).startswith("netG_A_a") for w in written)
    img = np.array(Image.open(written[0]))
    assert img.shape == (size, size) and img.dtype == np.uint8 and img.std() > 0


def test_train_and_test_clis_on_cpu(tmp_path):
    """train.py for one epoch of two steps, then test.py --General.inference netG_A on its checkpoints: checkpoint names, metrics.csv
    columns, the written translations."""
    import test as test_cli
    import train as train_cli
    root, out = str(tmp_path / "data"), str(tmp_path / "results")
    png_dataset(root)
    cfg_path = str(tmp_path / "cfg.yml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(cli_config(root, out), f)
    run = train_cli.main(["--config_file", cfg_path, "--num_workers", "0"])
    written = test_cli.main(["--config_file", os.path.join(run, "config.yml"), "--epoch", "latest", "--num_workers", "0"])
    check_cli_run(run, written, 32)


def test_shipped_config_builds_the_model_with_the_experiments_settings():
    """configs/config_cycle_gan.yml: the settings of the reference's experiment, a model section that define_model resolves, and a
    training chain of registered transforms with separate flip / rot90 entries for real_A and for real_B + background."""
    from octa_autosegmentation_amd.data import data_transforms as T
    from octa_autosegmentation_amd.models.cycle_gan import CycleGAN
    from octa_autosegmentation_amd.models.model import define_model
    from octa_autosegmentation_amd.utils.enums import Phase
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "config_cycle_gan.yml")))
    gen, tr = cfg["General"], cfg["Train"]
    assert (gen["task"], gen["inference"], gen["amp"]) == ("gan-ves-seg", "netG_A", True)
    assert {k: gen["model"][k] for k in ("lambda_A", "lambda_B", "lambda_idt", "pool_size")} == {"lambda_A": 10, "lambda_B": 10, "lambda_idt": 1, "pool_size": 50}
    assert (tr["lr"], tr["epochs"], tr["epochs_decay"], tr["batch_size"]) == (0.0002, 100, 0, 4)
    assert (tr["loss_criterionGAN"], tr["loss_criterionCycle"], tr["loss_criterionIdt"]) == ("LSGANLoss", "L1Loss", "L1Loss")
    chain = tr["data_augmentation"]
    names = [(a["name"], tuple(a["keys"])) for a in chain]
    for name in ("RandFlipd", "RandRotate90d"):
        assert (name, ("real_A",)) in names and (name, ("real_B", "background")) in names
    assert ("RandRotated", ("real_A", "real_B", "background")) in names
    load = [a for a in chain if a["name"] == "LoadGraphAndFilterByRandomRadiusd"][0]
    assert load["image_resolutions"] == [[304, 304]] and load["max_dropout_prob"] == 0.02
    assert cfg["Test"]["data_augmentation"][-2] == {"name": "AddRandomBackgroundNoised", "keys": ["real_A"]}
    for a in chain + cfg["Test"]["data_augmentation"]:
        assert hasattr(T, a["name"]), a["name"]
    cfg["General"]["device"] = "cpu"
    model = define_model(deepcopy(cfg), Phase.TRAIN)
    assert isinstance(model, CycleGAN) and model.fake_A_pool.pool_size == 50 and all(getattr(model, n) is not None for n in mk.NETS)
