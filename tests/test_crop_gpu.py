"""GPU: the Giarratano set-up -- the window form of the rotate kernel (csrc/augment.hip, octa_flip_rot90_rotate_window) against the
full-frame kernel, RandCropOrPadd on device tensors against the reference's recorded outputs, the fused batch loader against the
per-sample chain on configs/config_ves_seg-S_Giarratano.yml, the network at 360 x 360 (odd 45 x 45 bottleneck), and train.py / test.py /
validate.py with that config."""
import glob
import os
import random
import sys

import numpy as np
import pytest
import torch
import yaml

import _crop_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
CONFIG = os.path.join(ROOT, "configs", "config_ves_seg-S_Giarratano.yml")
SENTINEL = -7.25
GUARD = 4096          # sentinel floats in front of and behind the window kernel's output


# ---- 1. the window kernel against the full-frame kernel ---------------------------------------------------------------------------------

def _window_into_guarded_buffer(x, ang, k, f, thr, size, oy, ox):
    """octa_flip_rot90_rotate_window writing into the middle of a sentinel-filled buffer. -> (window [B, h, w], the guards)."""
    from octa_autosegmentation_amd import _native
    B, N = x.shape[0], x.shape[1]
    n = B * size[0] * size[1]
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=x.device)
    out = buf[GUARD:GUARD + n]
    _native.launch("octa_flip_rot90_rotate_window", x.device, x, out, B, N, ang, k, f, float(thr if thr is not None else 0.0), 0 if thr is None else 1,
                   size[0], size[1], oy, ox)
    torch.cuda.synchronize()
    return out.view(B, size[0], size[1]).clone(), torch.cat([buf[:GUARD], buf[GUARD + n:]])


# (N, (out_h, out_w), per-image (oy, ox)); B = 3
KERNEL_CASES = {
    "corner00": (37, (13, 20), [(0, 0)] * 3),
    "corner_far": (37, (13, 20), [(37 - 13, 37 - 20)] * 3),
    "interior": (37, (13, 20), [(3, 11), (17, 2), (9, 9)]),
    "block_seam": (300, (280, 290), [(0, 0), (20, 10), (7, 3)]),          # x crosses the 256-thread block seam
    "pad": (37, (48, 48), [(-5, -5)] * 3),                                  # (48 - 37) // 2 = 5
    "identity": (37, (37, 37), [(0, 0)] * 3),
}


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_window_kernel_equals_the_slice_of_the_full_frame_kernel(name, hip_lib_built):
    """Bit for bit, for all four rot_k, both flips, three angles in +-0.1745, threshold off / 0.1 / 0 (at 0 the padding becomes 1: the pad zero
    goes through the threshold), and nothing is written outside the window."""
    import torch.nn.functional as F
    from octa_autosegmentation_amd.data import gpu_augment as A
    N, size, offs = KERNEL_CASES[name]
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(N * 1000 + size[0])
    x = torch.rand((3, N, N), generator=g).to(dev)
    ang = torch.tensor([0.1745, -0.093, 0.031], dtype=torch.float32, device=dev)
    oy = torch.tensor([o[0] for o in offs], dtype=torch.int32, device=dev)
    ox = torch.tensor([o[1] for o in offs], dtype=torch.int32, device=dev)
    P = 64                                              # zero extension of the full frame on every side
    for k0 in range(4):
        for f0 in range(2):
            k = torch.tensor([(k0 + b) % 4 for b in range(3)], dtype=torch.int32, device=dev)
            f = torch.tensor([(f0 + b) % 2 for b in range(3)], dtype=torch.int32, device=dev)
            for thr in (None, 0.1, 0.0):
                full = A.flip_rot90_rotate(x, ang, k, f, thr)
                outside = 0.0 if thr is None else float(0.0 >= thr)
                ext = F.pad(full, (P, P, P, P), value=outside)
                want = torch.stack([ext[b, P + oy_b:P + oy_b + size[0], P + ox_b:P + ox_b + size[1]] for b, (oy_b, ox_b) in enumerate(offs)])
                got, guards = _window_into_guarded_buffer(x, ang, k, f, thr, size, oy, ox)
                assert torch.equal(got, want), (name, k0, f0, thr, float((got - want).abs().max()))
                assert bool((guards == SENTINEL).all()), (name, k0, f0, thr)
                assert torch.equal(A.flip_rot90_rotate_window(x, ang, k, f, thr, size, oy, ox), want)
                if name == "pad":                       # rows / columns 0..4 and 42..47 lie outside the 37 x 37 frame
                    assert bool((got[:, :5] == outside).all()) and bool((got[:, :, 42:] == outside).all()) and outside == (1.0 if thr == 0.0 else 0.0)


def test_window_kernel_without_rot_k_and_flip_tables(hip_lib_built):
    from octa_autosegmentation_amd.data import gpu_augment as A
    dev = torch.device("cuda")
    x = torch.rand((2, 37, 37), generator=torch.Generator().manual_seed(1)).to(dev)
    ang = torch.tensor([0.05, -0.17], dtype=torch.float32, device=dev)
    oy, ox = torch.tensor([4, 20], dtype=torch.int32, device=dev), torch.tensor([16, 0], dtype=torch.int32, device=dev)
    full = A.flip_rot90_rotate(x, ang)
    got = A.flip_rot90_rotate_window(x, ang, None, None, None, (13, 20), oy, ox)
    assert torch.equal(got, torch.stack([full[0, 4:17, 16:36], full[1, 20:33, 0:20]]))


def test_window_entry_point_refuses_bad_arguments(hip_lib_built):
    """An error code and a message, not a launch: the output keeps its sentinel."""
    from octa_autosegmentation_amd import _native
    dev = torch.device("cuda")
    x = torch.rand((2, 16, 16), device=dev)
    out = torch.full((2, 8, 8), SENTINEL, device=dev)
    ang = torch.zeros(2, device=dev)
    o = torch.zeros(2, dtype=torch.int32, device=dev)
    lib, ctx, stream = _native.lib(), _native.ctx(dev.index), _native.current_stream_ptr()
    p = lambda t: t.data_ptr() if t is not None else None
    call = lambda *a: lib.octa_flip_rot90_rotate_window(ctx, *a, stream)
    good = [p(x), p(out), 2, 16, p(ang), None, None, 0.0, 0, 8, 8, p(o), p(o)]

    def bad(i, v):
        a = list(good)
        a[i] = v
        return a

    for args in (bad(9, 0), bad(10, 0), bad(9, 65536), bad(10, 65536), bad(2, 0), bad(3, 0), bad(3, 65536), bad(11, None), bad(12, None), bad(0, None),
                 bad(1, None), bad(4, None), bad(1, p(x))):
        assert call(*args) == -2
        assert lib.octa_last_error().decode() == "octa_flip_rot90_rotate_window: bad arguments"
    assert lib.octa_flip_rot90_rotate_window(None, *good, stream) == -2
    with pytest.raises(_native.OctaHipError):
        _native.launch("octa_flip_rot90_rotate_window", dev, x, out, 2, 16, ang, None, None, 0.0, 0, 0, 8, o, o)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert call(*good) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, x[:, :8, :8])                    # angle 0, no flip, no turn: the window is the input's


# ---- 2. the transform on device tensors -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.CASES)
def test_rand_crop_or_pad_on_device_tensors_is_the_reference_bit_for_bit(name):
    C.check_case(name, "cuda")


# ---- 3. fused batch loader against the per-sample chain ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def graphs(tmp_path_factory, hip_lib_built):
    """Eight short seeded samples written by the generator CLI (the fixture of tests/test_training_cli_gpu.py)."""
    import generate_vessel_graph
    from octa_autosegmentation_amd.utils import configs
    cfg = configs.load_generator_config()
    out = tmp_path_factory.mktemp("graphs")
    modes = [dict(cfg["Greenhouse"]["modes"][0], I=30), dict(cfg["Greenhouse"]["modes"][1], I=20)]
    generate_vessel_graph.main(["--config_file", configs.GENERATOR_CONFIG, "--num_samples", "8", "--seed", "100", "--labels",
                                "--output.directory", str(out), "--Greenhouse.modes", yaml.safe_dump(modes, default_flow_style=True).strip()])
    dirs = sorted(glob.glob(str(out / "*")))
    assert len(dirs) == 8
    return str(out), dirs


def _run_loader(cfg, generic, monkeypatch):
    """One epoch of the Train loader. -> (batches, random.random() afterwards, the crop offsets [(oy, ox)] in sample order, the loader)."""
    from octa_autosegmentation_amd.data import data_transforms as T
    from octa_autosegmentation_amd.data.image_dataset import get_dataset
    taken = []

    class Spy(T.RandCropOrPadd):
        def __call__(self, data):
            data = super().__call__(data)
            taken.append(self.offsets)
            return data

    Spy.__name__ = "RandCropOrPadd"
    monkeypatch.setitem(T.TRANSFORMS, "RandCropOrPadd", Spy)
    cfg["General"]["generic_loader"] = generic
    torch.manual_seed(5); random.seed(5)
    loader = get_dataset(cfg, "Train", num_workers=0)
    assert (loader.fused is None) == generic and len(loader) == 2
    batches = []
    for b in loader:
        batches.append(b)
        if not generic and "crop_oy" in loader.fused.last_params:
            taken.extend(zip(loader.fused.last_params["crop_oy"].tolist(), loader.fused.last_params["crop_ox"].tolist()))
    return batches, random.random(), taken


def test_fused_batch_loader_with_the_crop_equals_the_per_sample_chain(graphs, monkeypatch):
    """configs/config_ves_seg-S_Giarratano.yml's training chain, fused against generic as tests/test_training_cli_gpu.py does for the S config:
    same paths, same offsets, same final state of `random`; images within that test's 1e-3; a label pixel of the window differs only where the
    two loaders' FULL frames (the chain without the crop entry) differ too, and those stay under that test's 1e-4 share; the fused window is
    the slice of the fused full frame, bit for bit."""
    out, dirs = graphs
    cfg = yaml.safe_load(open(CONFIG))
    csvs = os.path.join(out, "**", "*.csv")
    cfg["Train"]["data"] = {"image": {"files": csvs}, "label": {"files": csvs}}
    cfg["General"].update(amp=False, seed=11)
    fused, r_f, off_f = _run_loader(cfg, False, monkeypatch)
    plain, r_p, off_p = _run_loader(cfg, True, monkeypatch)
    assert r_f == r_p
    assert len(off_f) == len(off_p) == 8 and [tuple(o) for o in off_f] == [tuple(o) for o in off_p]
    assert len(set(off_f)) > 1 and all(0 <= oy <= 1216 - 360 and 0 <= ox <= 1216 - 360 for oy, ox in off_f)
    aug = cfg["Train"]["data_augmentation"]
    cfg["Train"]["data_augmentation"] = [d for d in aug if d["name"] != "RandCropOrPadd"]
    assert len(cfg["Train"]["data_augmentation"]) == len(aug) - 1
    fused_full, _, none_f = _run_loader(cfg, False, monkeypatch)
    plain_full, _, none_p = _run_loader(cfg, True, monkeypatch)
    assert none_f == none_p == []
    for i, (a, b, fa, fb) in enumerate(zip(fused, plain, fused_full, plain_full)):
        assert a["image_path"] == b["image_path"] == fa["image_path"] == fb["image_path"] and a["label_path"] == b["label_path"]
        assert a["image"].shape == b["image"].shape == a["label"].shape == b["label"].shape == (4, 1, 360, 360)
        assert a["image"].dtype == b["image"].dtype == torch.float32
        assert fa["image"].shape == fb["image"].shape == (4, 1, 1216, 1216)
        assert (a["image"] - b["image"]).abs().max().item() <= 1e-3
        assert set(a["label"].unique().tolist()) <= {0.0, 1.0}
        assert (fa["label"] != fb["label"]).float().mean().item() < 1e-4
        for s, (oy, ox) in enumerate(off_f[4 * i:4 * i + 4]):
            win = (slice(None), slice(oy, oy + 360), slice(ox, ox + 360))
            assert torch.equal(a["image"][s], fa["image"][s][win]) and torch.equal(a["label"][s], fa["label"][s][win])
            differ, differ_full = a["label"][s] != b["label"][s], (fa["label"][s] != fb["label"][s])[win]
            assert not bool((differ & ~differ_full).any())
    assert 0.005 < torch.cat([a["label"] for a in fused]).mean().item() < 0.6


# ---- 4. the network at the set-up's size ------------------------------------------------------------------------------------------------

def _model_kwargs():
    kw = dict(yaml.safe_load(open(CONFIG))["General"]["model"])
    assert kw.pop("name") == "DynUNet"
    return kw


def test_dynunet_logits_at_360_match_cpu_fp32():
    """fp32 without grad (the test.py / validate.py path) at 360 x 360, the smallest size with the set-up's odd 45 x 45 bottleneck, under
    OCTA_STRICT=1: within 1e-4 of the CPU fp32 modules, the bound of tests/test_models_gpu.py for this path."""
    from octa_autosegmentation_amd.models import networks
    assert os.environ.get("OCTA_STRICT") == "1"
    torch.manual_seed(0)
    net = networks.DynUNet(**_model_kwargs())
    networks.init_weights(net, init_type="kaiming", nonlinearity="leaky_relu")
    x = torch.rand(1, 1, 360, 360)
    before = networks.PATH_COUNTS["vendor"]
    with torch.no_grad():
        ref = net(x)
        got = net.cuda()(x.cuda()).cpu()
    err = float((got - ref).abs().max())
    print(f"DynUNet fp32 360x360: max |gpu - cpu| = {err:.3e}, max |cpu| = {float(ref.abs().max()):.3e}")
    assert networks.PATH_COUNTS["vendor"] == before
    assert torch.allclose(got, ref, atol=1e-4, rtol=1e-4), err


def test_training_steps_bf16_at_360_run_on_the_mfma_kernels():
    """Two optimiser steps at 2 x 1 x 360 x 360 under bf16 autocast and OCTA_STRICT=1: no vendor fallback, the MFMA path counted, finite losses."""
    from octa_autosegmentation_amd.models import networks
    from octa_autosegmentation_amd.models.segmentation_trainer import SegmentationTrainer
    assert os.environ.get("OCTA_STRICT") == "1"
    cfg = yaml.safe_load(open(CONFIG))
    torch.manual_seed(1)
    tr = SegmentationTrainer({"General": {"amp": True, "model": cfg["General"]["model"]},
                              "Train": {"lr": 1e-4, "loss": "DiceBCELoss", "epochs": 30, "epochs_decay": 10}}, "cuda")
    x = torch.rand(2, 1, 360, 360, device="cuda")
    y = (x > 0.7).float()
    before = dict(networks.PATH_COUNTS)
    for _ in range(2):
        _, losses = tr.perform_training_step({"image": x, "label": y})
        assert np.isfinite(float(losses["DiceBCELoss"].detach()))
    assert networks.PATH_COUNTS["vendor"] == before.get("vendor", 0) and networks.PATH_COUNTS["mfma"] > before.get("mfma", 0)


# ---- 5. the command-line tools with the new config --------------------------------------------------------------------------------------

def _pngs_360(graph_dirs, root):
    """Validation / test stand-ins at the dataset's size: the generated images and labels resampled to 360 x 360, as flat PNG folders."""
    from PIL import Image
    for sub in ("images", "labels"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    for i, d in enumerate(graph_dirs):
        name = os.path.basename(d)
        Image.open(os.path.join(d, "art_ven_img_gray.png")).resize((360, 360), Image.BILINEAR).save(os.path.join(root, "images", f"{i}.png"))
        Image.open(os.path.join(d, name + "_label.png")).convert("L").resize((360, 360), Image.NEAREST).save(os.path.join(root, "labels", f"{i}.png"))


def test_train_test_validate_with_the_giarratano_config(graphs, tmp_path):
    """train.py --config_file configs/config_ves_seg-S_Giarratano.yml for one epoch on the eight graphs (fused loader, 360 x 360 crops), then
    test.py and validate.py on its checkpoint with 360 x 360 PNGs. Only paths, the epoch count and the seed are overridden."""
    from PIL import Image
    import test as test_cli
    import train as train_cli
    import validate as validate_cli
    assert os.environ.get("OCTA_STRICT") == "1"
    out, dirs = graphs
    data = str(tmp_path / "png")
    _pngs_360(dirs, data)
    csvs = os.path.join(out, "**", "*.csv")
    f = lambda p: yaml.safe_dump({"files": p}, default_flow_style=True).strip()
    ov = ["--Train.data.image.files", csvs, "--Train.data.label.files", csvs, "--Train.epochs", "1", "--Train.epochs_decay", "0",
          "--Validation.data.image", f(os.path.join(data, "images", "*.png")), "--Validation.data.label", f(os.path.join(data, "labels", "*.png")),
          "--Test.data.image", f(os.path.join(data, "images", "*.png")), "--Output.save_dir", str(tmp_path / "results"), "--General.seed", "3"]
    run = train_cli.main(["--config_file", CONFIG] + ov)
    rows = open(os.path.join(run, "metrics.csv")).read().splitlines()
    assert rows[0].startswith("epoch,train_DiceBCELoss,val_DiceBCELoss,Train_DSC,Train_IoU,Validation_DSC,Validation_IoU") and len(rows) == 2
    vals = dict(zip(rows[0].split(","), (float(v) for v in rows[1].split(","))))
    assert np.isfinite(list(vals.values())).all() and 0 < vals["train_DiceBCELoss"] < 2
    assert "best_model_model.pth" in os.listdir(os.path.join(run, "checkpoints"))
    run_cfg = os.path.join(run, "config.yml")
    written = test_cli.main(["--config_file", run_cfg, "--epoch", "best", "--num_samples", "3"])
    assert len(written) == 3
    for w in written:
        pred = np.array(Image.open(w))
        assert pred.shape == (360, 360) and set(np.unique(pred)) <= {0, 255}
    metrics = validate_cli.main(["--config_file", run_cfg, "--epoch", "best"])
    assert {"Validation_DSC", "Validation_IoU"} <= set(metrics) and all(np.isfinite(v) for v in metrics.values())
