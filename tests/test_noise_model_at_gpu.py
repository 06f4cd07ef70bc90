"""GPU: the backward of the noise model (csrc/noise_model.hip octa_noise_model_backward, data/gpu_augment.py noise_model_rsample) and the
adversarial-augmentation loop on it (models/noise_model_at.py, configs/config_ves_seg-S_AA.yml).

Oracles: torch._dirichlet_grad in float64 on the CPU for the per-pixel reparameterised Beta gradient, float64 CPU autograd of the noise
model's formula for the whole backward; allowed is four times what torch's own float32 CPU evaluation deviates from the same float64 value,
measured in the test (the convention of tests/test_noise_model_gpu.py). Measured figures: DESIGN.md 4.2j."""
import os
import random
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

import _noise_model_cases as C
from test_noise_model_gpu import constant_grids
from test_training_cli_gpu import _pngs, graphs  # noqa: F401  (the eight generated graphs, a module-scoped fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
SIDE = 256
LARGE_PAIRS = [((2, 2), (0.5, 0.5)), ((8, 1), (1, 8)), ((0.5, 3), (5, 0.5))]
SMALL_PAIRS = [((1e-3, 2), (0.05, 0.05)), ((1e-3, 1e-3), (1e-3, 1e-3))]
CASES = [((40, 56), ("a_0", "a_1", "c_0"), (1, 0.7, 0.3)), ((96, 128), ("b_0", "b_1", "a_0"), (0.8, 0.5, 0.2))]


@pytest.fixture(scope="module")
def dev(hip_lib_built):
    assert os.environ.get("OCTA_STRICT") == "1"
    return torch.device("cuda", torch.cuda.current_device())


def beta_grad_cpu(t, a, b, dtype):
    """(dx/da, dx/db) of the Beta(a, b) variate of log-odds t as torch.distributions.Beta.rsample back-propagates them, by torch on the CPU in
    `dtype`: torch._dirichlet_grad on (x, 1 - x) = (1 / (1 + e^-t), 1 / (1 + e^t)) formed in float64 and rounded to dtype, then
    _Dirichlet_backward's projection g (go - sum(x go)) with go = (1, 0). Also the float64 x and 1 - x."""
    t64 = t.detach().cpu().double()
    x64, xc64 = 1 / (1 + torch.exp(-t64)), 1 / (1 + torch.exp(t64))
    xv = torch.stack([x64, xc64], -1).to(dtype)
    conc = torch.stack([a.detach().cpu().double(), b.detach().cpu().double()], -1).to(dtype)
    g = torch._dirichlet_grad(xv, conc, conc.sum(-1, keepdim=True).expand_as(conc))
    go = torch.tensor([1.0, 0.0], dtype=dtype)
    g = g * (go - (xv * go).sum(-1, keepdim=True))
    return g[..., 0], g[..., 1], x64, xc64


# ---- 1. the per-pixel reparameterised Beta gradient -------------------------------------------------------------------------------

def _bgrad(dev, pairs, seed):
    from octa_autosegmentation_amd.data import gpu_augment
    z = torch.zeros(1, SIDE, SIDE, device=dev)
    dgrids, extra = gpu_augment.noise_model_backward(z, z, z, constant_grids([pairs[0]], [pairs[1]]), seed, return_intermediates=True)
    return dgrids, extra


@pytest.mark.parametrize("pairs", LARGE_PAIRS)
def test_beta_gradient_per_pixel(dev, pairs):
    _, extra = _bgrad(dev, pairs, 0xBE7A0000 + LARGE_PAIRS.index(pairs))
    for k, pair in enumerate(pairs):
        t, a, b = extra["logodds"][0, k], extra["maps"][0, 2 * k], extra["maps"][0, 2 * k + 1]
        got = [extra["bgrad"][0, 2 * k].cpu().double(), extra["bgrad"][0, 2 * k + 1].cpu().double()]
        assert all(torch.isfinite(g).all() for g in got)
        da64, db64, x64, xc64 = beta_grad_cpu(t, a, b, torch.float64)
        da32, db32, _, _ = beta_grad_cpu(t, a, b, torch.float32)
        keep = torch.minimum(x64, xc64) >= 2.0 ** -20
        excluded = 1 - keep.double().mean().item()
        assert excluded <= 0.01, (pair, excluded)
        for name, g, g32, g64 in (("dx/da", got[0], da32, da64), ("dx/db", got[1], db32, db64)):
            rel = lambda v: ((v.double() - g64).abs() / g64.abs().clamp_min(1e-6))[keep].max().item()
            err, yard = rel(g), rel(g32)
            print(f"[beta gradient] Beta{pair} {name}: kernel vs float64 {err:.3e}, torch float32 vs float64 {yard:.3e}, excluded {excluded:.4f}", flush=True)
            assert yard > 0 and err <= 4 * yard, (pair, name, err, yard)


@pytest.mark.parametrize("pairs", SMALL_PAIRS)
def test_beta_gradient_small_shapes_are_finite(dev, pairs):
    dgrids, extra = _bgrad(dev, pairs, 0x5A110000 + SMALL_PAIRS.index(pairs))
    for v in (dgrids, extra["bgrad"], extra["dmaps"], extra["logodds"].nan_to_num(posinf=0, neginf=0), extra["out"]):
        assert torch.isfinite(v).all()


# ---- 2. the whole backward against autograd -----------------------------------------------------------------------------------------

class _BetaFromKernel(torch.autograd.Function):
    """The kernel's variate x as a function of the shape maps: forward returns x as the kernel drew it, backward is torch._dirichlet_grad at
    the kernel's emitted (t, A, B)."""

    @staticmethod
    def forward(ctx, a, b, x, t, ka, kb):
        ctx.grads = beta_grad_cpu(t, ka, kb, a.dtype)[:2]
        return x.to(a.dtype)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.grads[0], g * ctx.grads[1], None, None, None, None


def formula(img, bg, grids, lambdas, dtype, delta=None, n=None, drawn=None):
    """tests/_noise_model_cases.py evaluate (which detaches its inputs) with the graph kept: -> (out, leaf grids, raw maps). drawn =
    (fields [B,2,H,W], logodds [B,2,H,W], maps [B,5,H,W]) of the kernel replaces an injected field by _BetaFromKernel."""
    ld, ls, lg = lambdas
    img, bg = img.detach().cpu().to(dtype), bg.detach().cpu().to(dtype)
    leaf = grids.detach().cpu().to(dtype).requires_grad_(True)
    g5 = torch.cat([leaf[:, :4], torch.clamp(leaf[:, 4:], 0, 1) * (2 * lg) + (1 - lg)], dim=1)
    raw = F.interpolate(g5, img.shape[-2:], mode="bicubic")
    maps = torch.cat([torch.clamp(raw[:, :4], min=1e-3), raw[:, 4:]], dim=1)
    field = []
    for k, given in enumerate((delta, n)):
        if given is not None:
            field.append(given.detach().cpu().to(dtype))
        else:
            f, t, km = (v.detach().cpu() for v in drawn)
            field.append(_BetaFromKernel.apply(maps[:, 2 * k], maps[:, 2 * k + 1], f[:, k], t[:, k], km[:, 2 * k], km[:, 2 * k + 1]))
    x = torch.maximum(img, bg * ld * field[0])
    x = x * (ls * field[1] + (1 - ls))
    return torch.pow(x + 1e-6, maps[:, 4]), leaf, raw


def _case(shape, names, variant):
    g = C.golden()
    gen = torch.Generator().manual_seed(shape[0] + 17)
    B = len(names)
    img, bg, delta, n, dout = (torch.rand((B,) + shape, generator=gen) for _ in range(5))
    dout = dout * 2 - 1
    grids = torch.stack([torch.from_numpy(g[f"{k}_grids"].copy()) for k in names])
    if variant == "masks":          # gamma control points outside [0, 1] (no gradient) and exactly on both ends (gradient: torch.clamp's mask is closed)
        grids[:, 4, ::2, 1::3] = 1.25
        grids[:, 4, 1::2, ::3] = -0.5
        grids[:, 4, 4, 5], grids[:, 4, 3, 5] = 0.0, 1.0
    return img, bg, delta, n, dout, grids


def _grad(out, leaf, dout):
    (out * dout.to(out.dtype)).sum().backward()
    return leaf.grad.double()


def _compare(what, got, g32, g64):
    for k, name in enumerate(("alpha_v", "beta_v", "alpha_s", "beta_s", "gamma")):
        err, yard = (got[:, k].cpu().double() - g64[:, k]).abs().max().item(), (g32[:, k] - g64[:, k]).abs().max().item()
        print(f"[noise model backward, {what}] dGrids {name}: kernel vs float64 {err:.3e}, torch float32 vs float64 {yard:.3e}, "
              f"largest |gradient| {g64[:, k].abs().max().item():.3e}", flush=True)
        if g64[:, k].abs().max().item() == 0:
            assert got[:, k].abs().max().item() == 0, name
        else:
            assert yard > 0 and err <= 4 * yard, (what, name, err, yard)


@pytest.mark.parametrize("variant", ["plain", "masks"])
@pytest.mark.parametrize("shape, names, lambdas", CASES)
def test_backward_with_injected_fields_against_autograd(dev, shape, names, lambdas, variant):
    """Delta and N injected: no sampler term, the shape grids get exactly 0 and the gamma grid the gradient of pow through the bicubic map,
    the factor 2 lambda_gamma and the closed clamp mask."""
    from octa_autosegmentation_amd.data import gpu_augment
    img, bg, delta, n, dout, grids = _case(shape, names, variant)
    out64, leaf64, _ = formula(img, bg, grids, lambdas, torch.float64, delta, n)
    assert torch.equal(out64.detach(), C.evaluate(img, bg, grids, delta, n, lambdas, torch.float64)[0])
    out32, leaf32, _ = formula(img, bg, grids, lambdas, torch.float32, delta, n)
    g64, g32 = _grad(out64, leaf64, dout), _grad(out32, leaf32, dout)
    to = lambda v: v.to(dev)
    got = gpu_augment.noise_model_backward(to(dout), to(img), to(bg), grids, 7, *lambdas, delta=to(delta), n=to(n))
    assert got.shape == grids.shape and got.dtype == torch.float32
    if variant == "masks":
        assert (g64[:, 4, ::2, 1::3] == 0).all() and g64[:, 4, 4, 5].abs().min() > 0 and g64[:, 4, 3, 5].abs().min() > 0
        assert (got[:, 4, ::2, 1::3] == 0).all() and (got[:, 4, 1::2, ::3] == 0).all()
    _compare(f"injected, {variant}, {shape}", got, g32, g64)
    # the same through the autograd binding
    leaf = grids.to(dev).requires_grad_(True)
    out = gpu_augment.noise_model_rsample(to(img), to(bg), leaf, 7, *lambdas, delta=to(delta), n=to(n))
    (out * to(dout)).sum().backward()
    assert torch.equal(leaf.grad, got)


@pytest.mark.parametrize("shape, names, lambdas", CASES)
def test_backward_with_drawn_fields_against_autograd(dev, shape, names, lambdas):
    """Drawn Delta and N: the sampler term through the reparameterised Beta gradient, the maximum's branch and (first case: lambda_delta 1,
    background 1 there, image = the drawn Delta) its exact ties, the 1e-3 clamp of the shape maps."""
    from octa_autosegmentation_amd.data import gpu_augment
    img, bg, _, _, dout, grids = _case(shape, names, "plain")
    seed, to = 0xD0A3 + shape[0], lambda v: v.to(dev)
    fields = gpu_augment.noise_model(to(img), to(bg), grids, seed, *lambdas, return_fields=True)[2].cpu()
    if lambdas[0] == 1:
        bg[:, 5:15, 5:25] = 1.0
        img[:, 5:15, 5:25] = fields[:, 0, 5:15, 5:25]           # the draws do not depend on the image: these pixels tie exactly
    got, extra = gpu_augment.noise_model_backward(to(dout), to(img), to(bg), grids, seed, *lambdas, return_intermediates=True)
    kernel = (fields, extra["logodds"], extra["maps"])
    out64, leaf64, raw64 = formula(img, bg, grids, lambdas, torch.float64, drawn=kernel)
    out32, leaf32, _ = formula(img, bg, grids, lambdas, torch.float32, drawn=kernel)
    d, i = bg.double() * lambdas[0] * fields[:, 0].double(), img.double()
    assert (raw64[:, :4] < 1e-3).any() and (raw64[:, :4] > 1e-3).any()          # the clamp, both sides
    assert (d > i).any() and (d < i).any() and ((d == i).sum().item() >= 3 * 200) == (lambdas[0] == 1)          # the maximum, both sides, ties
    assert (extra["maps"][:, :4].min().item() == np.float32(1e-3))
    g64, g32 = _grad(out64, leaf64, dout), _grad(out32, leaf32, dout)
    assert g64[:, :4].abs().max().item() > 0
    _compare(f"drawn, {shape}", got, g32, g64)


# ---- 3. a wrong tap -----------------------------------------------------------------------------------------------------------------

def test_gradient_lands_on_the_perturbed_control_point(dev):
    """A central difference of sum(out dOut) in ONE gamma control point (injected fields: the function is smooth in it) against dGrids there.
    Error of the difference quotient with step h = 0.01: truncation h^2 / 6 |f'''| <= 1e-5 |f'| (f''' / f' = (2 lambda_gamma w ln u)^2 <= 0.6^2
    14^2 w^2 with tap weights w well below 1), rounding: float32 outputs, 2240 terms of size <= 2 with 2^-24 relative error each, at most
    2240 * 2 * 2^-23 / (2 h) = 2.7e-2 in the worst case and ~6e-4 for independent errors. Allowed: 2e-3 (1 + |gradient|). dOut is a ramp across
    the columns, so the next control point's gradient is another number: it must miss by more than ten times that."""
    from octa_autosegmentation_amd.data import gpu_augment
    shape, names, lambdas = CASES[0]
    img, bg, delta, n, _, grids = _case(shape, names, "plain")
    grids[:, 4] = grids[:, 4] * 0.5 + 0.25                    # inside (0, 1): the clamp is not in the way of a finite step
    dout = torch.linspace(0.2, 3.0, shape[1]).expand(len(names), shape[0], shape[1]).contiguous()
    to = lambda v: v.to(dev)
    got = gpu_augment.noise_model_backward(to(dout), to(img), to(bg), grids, 7, *lambdas, delta=to(delta), n=to(n)).cpu().double()
    h, at, beside = 0.01, (1, 4, 4, 4), (1, 4, 4, 5)

    def f(step):
        gp = grids.clone()
        gp[at] += step
        out = gpu_augment.noise_model(to(img), to(bg), gp, 7, *lambdas, delta=to(delta), n=to(n))
        return (out.cpu().double() * dout.double()).sum().item()

    fd = (f(h) - f(-h)) / (2 * h)
    tol = 2e-3 * (1 + abs(fd))
    print(f"[wrong tap] central difference {fd:.6f}, dGrids there {got[at].item():.6f}, beside {got[beside].item():.6f}, allowed {tol:.2e}", flush=True)
    assert abs(got[at].item() - fd) <= tol
    assert abs(got[beside].item() - fd) > 10 * tol


# ---- 4. determinism -----------------------------------------------------------------------------------------------------------------

def test_backward_is_deterministic_and_batch_independent(dev):
    from octa_autosegmentation_amd.data import gpu_augment
    shape, names, lambdas = CASES[0]
    img, bg, _, _, dout, grids = (v.to(dev) for v in _case(shape, names, "plain"))
    seed = 0x0123456789ABCDEF
    a, ea = gpu_augment.noise_model_backward(dout, img, bg, grids, seed, *lambdas, return_intermediates=True)
    b, eb = gpu_augment.noise_model_backward(dout, img, bg, grids, seed, *lambdas, return_intermediates=True)
    assert torch.equal(a, b) and all(torch.equal(ea[k].nan_to_num(), eb[k].nan_to_num()) for k in ea)
    assert torch.isfinite(a).all() and a[:, :4].abs().max().item() > 0
    for s in range(len(names)):
        one, eo = gpu_augment.noise_model_backward(dout[s:s + 1], img[s:s + 1], bg[s:s + 1], grids[s:s + 1], seed, *lambdas, return_intermediates=True,
                                                   sample_offset=s)
        assert torch.equal(one, a[s:s + 1]) and torch.equal(eo["dmaps"], ea["dmaps"][s:s + 1])
    # the forward re-run inside the backward is the forward: the same output (so the same Delta and N) and the same maps, bit for bit
    out, maps, _ = gpu_augment.noise_model(img, bg, grids, seed, *lambdas, return_fields=True)
    assert torch.equal(ea["out"], out) and torch.equal(ea["maps"], maps)
    assert not torch.equal(gpu_augment.noise_model_backward(dout, img, bg, grids, seed + 1, *lambdas), a)


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------------

def _aa_config():
    return yaml.safe_load(open(os.path.join(ROOT, "configs", "config_ves_seg-S_AA.yml")))


def test_adversarial_loop_on_the_mfma_path(dev):
    """DynUNet of the S_AA config, frozen, on the hand-written kernels (OCTA_STRICT=1: a layer that left them would raise): the ascent loop
    leaves the network no gradient, moves the grids, and does not lower the loss against the same draws from unmoved grids (alpha = 0 under the
    same seeds: the same geometry, the same control points, the same four per-sample seeds); then one training step updates the weights."""
    from octa_autosegmentation_amd.models import networks
    from octa_autosegmentation_amd.models.noise_model_at import AtLoss
    from octa_autosegmentation_amd.models.segmentation_trainer import SegmentationTrainer
    torch.manual_seed(11)
    tr = SegmentationTrainer(_aa_config(), dev)
    gen = torch.Generator().manual_seed(12)
    x, bg = torch.rand(2, 1, 64, 64, generator=gen).to(dev), (torch.rand(2, 1, 64, 64, generator=gen) * 0.6).to(dev)
    y = (F.interpolate(x, size=(256, 256), mode="bilinear") > 0.6).float()
    model, at = tr.impl.model, tr.impl.at
    assert isinstance(at, AtLoss) and at.grad_scale == 65536.0
    before = dict(networks.PATH_COUNTS)

    def run(alpha):
        torch.manual_seed(21); random.seed(22)
        loop = AtLoss(at.loss_fun, alpha=alpha, autocast=tr.impl.autocast)
        adv, label = loop(model, x, bg, y)
        with torch.no_grad(), tr.impl.autocast():
            loss = loop.loss_fun(model(adv).float(), label.float()).item()
        return loop, adv, label, loss

    moved, adv, label, loss_moved = run(at.alpha)
    assert networks.PATH_COUNTS["vendor"] == before.get("vendor", 0) and networks.PATH_COUNTS["mfma"] > before.get("mfma", 0)
    assert all(p.grad is None and p.requires_grad for p in model.parameters())
    assert adv.shape == label.shape == (2, 1, 256, 256) and not adv.requires_grad and torch.isfinite(adv).all()
    change = (moved.grid_trajectory[3] - moved.grid_trajectory[0]).abs()
    still, _, label0, loss_still = run(0.0)
    assert torch.equal(still.grid_trajectory[3], still.grid_trajectory[0]) and torch.equal(still.grid_trajectory[0], moved.grid_trajectory[0])
    assert torch.equal(label0, label)
    print(f"[AT end to end] largest grid change {change.max().item():.3e}, loss on the sample of the moved grids {loss_moved:.6f}, of the unmoved grids "
          f"{loss_still:.6f}, losses inside the loop {[round(v.item(), 6) for v in moved.loss_trajectory]}", flush=True)
    assert torch.isfinite(moved.grid_trajectory[3]).all() and change.max().item() > 1e-4
    assert loss_moved >= loss_still
    w = model.input_block.conv1.conv.weight
    w0 = w.detach().clone()
    h = lambda t: t.to(torch.bfloat16)
    batch = {"image": h(x), "background": bg, "label": h(y)}      # the loader's CastToTyped hands image and label over in bf16 under amp
    _, losses = tr.perform_training_step(batch)
    assert np.isfinite(float(losses["DiceBCELoss"])) and not torch.equal(w.detach(), w0)
    assert networks.PATH_COUNTS["vendor"] == before.get("vendor", 0)


def test_loader_dtypes_give_the_float32_label(dev):
    """Under General.amp the loader delivers image and label in bf16 and the background in float32. The label's rotation must not inherit
    that dtype: a bf16 sampling grid has a quantum of 2 - 4 pixels at 1216^2. A label of thin lines (exact in bf16) at that size, through the
    loop in the loader's dtypes and, under the same seeds, in float32: the same label, bit for bit, label and sample float32; and the
    label is what torch's float32 rot90 + rotation + threshold give."""
    from octa_autosegmentation_amd.models.noise_model_at import AtLoss, rotate_bilinear
    from octa_autosegmentation_amd.models.segmentation_trainer import SegmentationTrainer
    torch.manual_seed(13)
    tr = SegmentationTrainer(_aa_config(), dev)
    gen = torch.Generator().manual_seed(14)
    x = torch.rand(2, 1, 304, 304, generator=gen).to(torch.bfloat16).to(dev)
    bg = (torch.rand(2, 1, 304, 304, generator=gen) * 0.6).to(dev)
    y = torch.zeros(2, 1, 1216, 1216)
    y[:, :, ::16] = 1.0
    y[:, :, 1::16] = 1.0
    y[:, :, :, 5::24] = 1.0
    y = y.to(dev)

    def run(image, label):
        torch.manual_seed(31)
        loop = AtLoss(tr.impl.at.loss_fun, autocast=tr.impl.autocast, seed=32)
        return loop, loop(tr.impl.model, image, bg, label)

    loop, (adv_h, label_h) = run(x, y.to(torch.bfloat16))
    _, (adv_f, label_f) = run(x.float(), y)
    assert label_h.dtype == adv_h.dtype == torch.float32 and label_h.shape == (2, 1, 1216, 1216)
    assert torch.equal(label_h, label_f) and adv_f.dtype == torch.float32          # (the samples: equal up to grid_sample's atomics in the loop's backward)
    want = torch.stack([rotate_bilinear(torch.rot90(y[b:b + 1], loop.rot_k[b], dims=(-2, -1)), loop.rot_r[b])[0] for b in range(2)])
    assert torch.equal(label_h, (want >= 0.1).float()) and 0.05 < label_h.mean().item() < 0.5


def test_train_cli_with_the_aa_config(dev, graphs, tmp_path):  # noqa: F811
    """One epoch of train.py --config_file configs/config_ves_seg-S_AA.yml on the eight graphs under OCTA_STRICT=1: only paths, the epoch
    count and the seed are overridden."""
    import train as train_cli
    out, dirs = graphs
    data = str(tmp_path / "png")
    _pngs(dirs, data)
    csvs = os.path.join(out, "**", "*.csv")
    f = lambda p: yaml.safe_dump({"files": p}, default_flow_style=True).strip()
    ov = ["--Train.data.image.files", csvs, "--Train.data.label.files", csvs, "--Train.data.background.files", os.path.join(data, "background", "*.png"),
          "--Train.epochs", "1", "--Train.epochs_decay", "0",
          "--Validation.data.image", f(os.path.join(data, "images", "*.png")), "--Validation.data.label", f(os.path.join(data, "labels", "*.png")),
          "--Test.data.image", f(os.path.join(data, "images", "*.png")), "--Output.save_dir", str(tmp_path / "results"), "--General.seed", "3"]
    run = train_cli.main(["--config_file", os.path.join(ROOT, "configs", "config_ves_seg-S_AA.yml")] + ov)
    rows = open(os.path.join(run, "metrics.csv")).read().splitlines()
    assert rows[0].startswith("epoch,train_DiceBCELoss") and len(rows) == 2
    vals = dict(zip(rows[0].split(","), (float(v) for v in rows[1].split(","))))
    assert np.isfinite(list(vals.values())).all() and 0 < vals["train_DiceBCELoss"] < 2
    assert "latest_model_model.pth" in os.listdir(os.path.join(run, "checkpoints"))
