"""GPU: the CycleGAN step on the bf16 / MFMA path (models/cycle_gan.py): two generators chained through each other, the
reference-made fixture on the device, the fused elementwise tail against the torch composition, and train.py / test.py end to end."""
import os
import random
import sys

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _three_way(net, x, target, passes):
    """One forward + backward of `net` three ways with the SAME bf16-rounded parameters: the torch modules in fp32 (the reference), the
    torch modules under bf16 autocast (the yardstick of what bf16 activations cost through this depth), and the product path (bf16
    autocast on the hand-written kernels, counted: `passes` network passes). Returns {way: (output, input gradient, {name: weight gradient})}."""
    from octa_autosegmentation_amd.models import networks
    res = {}
    for way in ("fp32", "autocast", "mfma"):
        net.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        before = networks.PATH_COUNTS["mfma"]
        if way == "mfma":
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = net(xi)
            assert networks.PATH_COUNTS["mfma"] == before + passes, "the bf16 pass did not take the hand-written kernels"
        else:
            with networks.vendor_reference(), torch.backends.cudnn.flags(enabled=False), torch.autocast("cuda", dtype=torch.bfloat16, enabled=way == "autocast"):
                old, networks.USE_MFMA_CONV = networks.USE_MFMA_CONV, False
                try:
                    y = net(xi)
                finally:
                    networks.USE_MFMA_CONV = old
            assert networks.PATH_COUNTS["mfma"] == before
        ((y.float() - target) ** 2).mean().backward()
        res[way] = (y.float().detach(), xi.grad.detach().float(), {k: p.grad.detach().float().clone() for k, p in net.named_parameters()
                                                                   if p.grad is not None and p.dim() == 4})
    return res


def _assert_within_bf16_budget(res, tag):
    """Per-tensor relative L2 error of the product path against the fp32 run: at most twice the torch-autocast run's own error + 1 %
    (output, input gradient and EVERY convolution weight gradient)."""
    ref, ac, got = res["fp32"], res["autocast"], res["mfma"]
    rows = [("output", _rel(got[0], ref[0]), _rel(ac[0], ref[0])), ("d/dx", _rel(got[1], ref[1]), _rel(ac[1], ref[1]))]
    assert set(got[2]) == set(ref[2]), "a convolution weight is missing its gradient on the product path"
    rows += [(k, _rel(got[2][k], ref[2][k]), _rel(ac[2][k], ref[2][k])) for k in ref[2] if ref[2][k].norm().item() > 1e-12]
    worst = max(rows, key=lambda r: r[1] - 2.0 * r[2])
    print(f"[{tag}] output {rows[0][1]:.4f} (torch autocast {rows[0][2]:.4f}), d/dx {rows[1][1]:.4f} ({rows[1][2]:.4f}), worst tensor {worst[0]}: "
          f"{worst[1]:.4f} ({worst[2]:.4f})", flush=True)
    for name, r_got, r_ac in rows:
        assert r_got <= 2.0 * r_ac + 0.01, (tag, name, r_got, r_ac)
    return rows


class _Chain(torch.nn.Module):
    def __init__(self, first, second):
        super().__init__()
        self.first, self.second = first, second

    def forward(self, x):
        return self.second(self.first(x))


@pytest.mark.parametrize("shape", [(2, 1, 32, 32), (1, 1, 48, 40)], ids=["2x32x32", "1x48x40"])
def test_chained_generators_on_the_mfma_path(shape, hip_lib_built):
    """G_B(G_A(x)): the first place where a generator's stem receives its gradient from another generator's head instead of from a
    loss. Output, input gradient and every convolution weight gradient of BOTH generators against an fp32 run of the torch modules on
    the same bf16-rounded He weights; 48 x 40 is not square, so a transposed stride in the stem's data gradient shows."""
    from octa_autosegmentation_amd.models import networks, weight_cache
    torch.manual_seed(3)
    net = _Chain(networks.resnetGenerator9(), networks.resnetGenerator9()).cuda()
    for g in (net.first, net.second):
        networks.init_weights(g, "kaiming", nonlinearity="relu")
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(p.to(torch.bfloat16).float())
    weight_cache.invalidate()
    x = torch.rand(shape, device="cuda").to(torch.bfloat16).float()
    target = torch.rand(shape, device="cuda")
    res = _three_way(net, x, target, passes=2)
    assert res["mfma"][0].shape == shape
    rows = _assert_within_bf16_budget(res, f"chain {shape}")
    assert sum(1 for r in rows if r[0].startswith("first.")) == sum(1 for r in rows if r[0].startswith("second.")) >= 20


def _device_steps(tag, steps, mfma):
    """`steps` steps of fixture variant `tag` on the device under bf16 autocast -> (losses [steps, 9], gradient norms [steps, 4])."""
    from octa_autosegmentation_amd.models import networks
    from tests.test_cycle_gan import build_model, golden, mk
    lambda_idt, pool_size, background = mk.VARIANTS[tag]
    ident = {"prediction": lambda t: t, "label": lambda t: t}
    old = networks.USE_MFMA_CONV
    try:
        if not mfma:
            networks.USE_MFMA_CONV = False
        model = build_model(lambda_idt, pool_size, device="cuda", amp=True)
        torch.manual_seed(mk.TORCH_SEED)
        random.seed(int(golden()[f"{tag}_random_seed"]))
        losses, norms = [], []
        before = networks.PATH_COUNTS["vendor"]
        for _ in range(steps):
            b = {k: v.cuda() for k, v in mk.batch(background).items()}
            if mfma:
                _, l = model.perform_training_step(b, None, ident, torch.device("cuda"))
            else:
                with networks.vendor_reference(), torch.backends.cudnn.flags(enabled=False):
                    _, l = model.perform_training_step(b, None, ident, torch.device("cuda"))
            losses.append([float(l[k]) for k in mk.LOSS_KEYS])
            norms.append(mk.grad_norms(model))
        assert networks.PATH_COUNTS["vendor"] == before
    finally:
        networks.USE_MFMA_CONV = old
    return np.array(losses), np.array(norms)


def test_fixture_on_the_device_bf16_mfma(hip_lib_built):
    """Fixture variant `bg` (lambda_idt 1, pool_size 2, background in the batch) through the product path: bf16 autocast, batched passes,
    MFMA generators and PatchGANs, the fused tail. OCTA_STRICT=1 (tests/conftest.py): a vendor kernel would raise. First-step losses and
    first-step gradient norms within twice the deviation that torch's own autocast run of the same model (torch modules, same seed, same
    device) shows from the fixture, plus 1 %. The uniform field is drawn on the device, so both runs differ from the CPU-made fixture by the
    same other draw. Later steps: finite only -- behind an optimiser step the bf16 runs leave fp32 at a rate nothing here derives."""
    from tests.test_cycle_gan import golden, mk
    assert os.environ.get("OCTA_STRICT") == "1"
    g = golden()
    want_l, want_g = g["bg_losses"][0], g["bg_grad_norms"][0]
    ac_l, ac_g = _device_steps("bg", 1, mfma=False)
    got_l, got_g = _device_steps("bg", mk.STEPS, mfma=True)
    dev = lambda a, w: np.abs(a - w) / np.abs(w)
    print(f"[cyclegan bg on device] first-step losses: mfma {np.round(dev(got_l[0], want_l), 4)} autocast {np.round(dev(ac_l[0], want_l), 4)}", flush=True)
    print(f"[cyclegan bg on device] first-step gradient norms: mfma {np.round(dev(got_g[0], want_g), 4)} autocast {np.round(dev(ac_g[0], want_g), 4)}", flush=True)
    assert (dev(got_l[0], want_l) <= 2.0 * dev(ac_l[0], want_l) + 0.01).all(), (got_l[0], ac_l[0], want_l)
    assert (dev(got_g[0], want_g) <= 2.0 * dev(ac_g[0], want_g) + 0.01).all(), (got_g[0], ac_g[0], want_g)
    assert np.isfinite(got_l).all() and np.isfinite(got_g).all()


def test_fused_tail_against_the_torch_composition(hip_lib_built):
    """One step with USE_FUSED_GAN_LOSS on and off, from the same state and seeds. The nine losses are float32 values of the same sums
    (the fused ones taken in double): 1e-5 relative. Every parameter gradient within the bf16 budget with the composed run as the
    reference: there is no third run whose own error could be doubled, which leaves the rule's 1 % of relative L2 error."""
    from octa_autosegmentation_amd.models import gan_loss
    from tests.test_cycle_gan import build_model, mk
    ident = {"prediction": lambda t: t, "label": lambda t: t}
    out = {}
    for fused in (False, True):
        old = gan_loss.USE_FUSED_GAN_LOSS
        gan_loss.USE_FUSED_GAN_LOSS = fused
        try:
            model = build_model(1.0, 2, device="cuda", amp=True)
            torch.manual_seed(1)
            random.seed(1)
            b = {k: v.cuda() for k, v in mk.batch(True).items()}
            _, l = model.perform_training_step(b, None, ident, torch.device("cuda"))
            out[fused] = (np.array([float(l[k]) for k in mk.LOSS_KEYS]),
                          {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None})
        finally:
            gan_loss.USE_FUSED_GAN_LOSS = old
    (l0, g0), (l1, g1) = out[False], out[True]
    print(f"[cyclegan fused vs composed] losses max rel dev {np.max(np.abs(l1 - l0) / np.abs(l0)):.2e}", flush=True)
    assert np.allclose(l1, l0, rtol=1e-5, atol=0), (l1, l0)
    assert set(g0) == set(g1) and len(g0) >= 40
    rows = [(n, _rel(g1[n], g0[n])) for n in g0 if g0[n].norm().item() > 1e-12]
    worst = max(rows, key=lambda r: r[1])
    print(f"[cyclegan fused vs composed] {len(rows)} gradients, worst {worst[0]}: {worst[1]:.4f}", flush=True)
    assert all({n.split(".")[0] for n, _ in rows} >= {net} for net in mk.NETS)
    for n, r in rows:
        assert r <= 0.01, (n, r)


def test_train_and_test_clis_on_the_device(tmp_path, hip_lib_built):
    """train.py for one epoch on the four-sample directory with `amp: true` on the device, then test.py --General.inference netG_A and the
    S_GAN route (ImageToImageTranslationd from the written netG_A checkpoint). OCTA_STRICT=1: no vendor kernel in the step."""
    import test as test_cli
    import train as train_cli
    from octa_autosegmentation_amd.data import data_transforms as T
    from octa_autosegmentation_amd.models import networks
    from tests.test_cycle_gan import check_cli_run, cli_config, png_dataset
    assert os.environ.get("OCTA_STRICT") == "1"
    root, out = str(tmp_path / "data"), str(tmp_path / "results")
    png_dataset(root)
    cfg_path = str(tmp_path / "cfg.yml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(cli_config(root, out, device="cuda:0", amp=True), f)
    before = dict(networks.PATH_COUNTS)
    run = train_cli.main(["--config_file", cfg_path, "--num_workers", "0"])
    assert networks.PATH_COUNTS["mfma"] >= before.get("mfma", 0) + 2 * 7 and networks.PATH_COUNTS["vendor"] == before.get("vendor", 0)
    written = test_cli.main(["--config_file", os.path.join(run, "config.yml"), "--epoch", "latest", "--num_workers", "0"])
    check_cli_run(run, written, 32)
    t = T.ImageToImageTranslationd(model_path=os.path.join(run, "checkpoints", "latest_netG_A_model.pth"), keys=["image"])
    y = t({"image": torch.rand(1, 32, 32, device="cuda")})["image"]
    assert y.shape == (1, 32, 32) and bool(torch.isfinite(y).all()) and 0.0 <= float(y.min()) and float(y.max()) <= 1.0
