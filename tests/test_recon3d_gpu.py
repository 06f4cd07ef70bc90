"""GPU: the 3-D reconstruction set-up end to end through the drop-in CLIs: graphs -> NIfTI label volumes (visualize_vessel_graphs.py),
a cut-down configs/config_3d_recon_supervised.yml through train.py under OCTA_STRICT=1, test.py writing NIfTI predictions."""
import copy
import csv
import glob
import os

import numpy as np
import pytest
import yaml

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = "48,48,13"          # 13 depth slices: SelectSlice [[5,-4]] keeps 4


@pytest.fixture(scope="module")
def graphs(tmp_path_factory, hip_lib_built):
    """Two small vessel graphs, made as tests/test_cli_gpu.py makes them -> (directory, [csv paths])."""
    import sys
    sys.path.insert(0, ROOT)
    import generate_vessel_graph
    g = np.load(os.path.join(ROOT, "tests", "golden", "sim_golden.npz"))
    cfg = yaml.safe_load(str(g["config_yaml"]))
    cfg["Greenhouse"]["modes"][0]["I"], cfg["Greenhouse"]["modes"][1]["I"] = 10, 5
    base = tmp_path_factory.mktemp("recon3d")
    cfg_path = base / "cfg.yml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    out_dir = base / "graphs"
    generate_vessel_graph.main(["--config_file", str(cfg_path), "--num_samples", "2", "--seed", "0", "--output.directory", str(out_dir)])
    files = sorted(glob.glob(str(out_dir / "*" / "*.csv")))
    assert len(files) == 2
    return base, files


@pytest.fixture(scope="module")
def volumes(graphs):
    """visualize_vessel_graphs.py --save_3d --binarize (NIfTI, the default) on the two graphs -> directory."""
    import visualize_vessel_graphs
    base, _ = graphs
    vol_dir = base / "volumes"
    visualize_vessel_graphs.main(["--source_dir", str(base / "graphs"), "--out_dir", str(vol_dir), "--resolution", RES, "--save_3d", "--binarize"])
    return vol_dir


def _forest(path):
    with open(path, newline="") as fh:
        return list(csv.DictReader(fh))


def test_visualize_writes_the_voxelised_volume_as_nifti(graphs, volumes):
    import visualize_vessel_graphs
    from octa_autosegmentation_amd import nifti
    from octa_autosegmentation_amd.vessel_graph_generation import tree2img
    base, files = graphs
    for path in files:
        name = os.path.basename(path)[:-4]
        want, _ = tree2img.voxelize_forest(_forest(path), [48, 48, 13])
        got, hdr = nifti.read(str(volumes / (name + "_3d_label.nii.gz")))
        assert got.dtype == want.dtype == np.uint16 and hdr["datatype"] == 512 and got.shape == want.shape == (48, 48, 13)
        assert np.array_equal(got, (want >= 1).astype(np.uint16)) and got.max() == 1
    # without --binarize: the voxeliser's own values; and .npy still works
    raw_dir, npy_dir = base / "volumes_raw", base / "volumes_npy"
    visualize_vessel_graphs.main(["--source_dir", str(base / "graphs"), "--out_dir", str(raw_dir), "--resolution", RES, "--save_3d", "--no_save_2d"])
    visualize_vessel_graphs.main(["--source_dir", str(base / "graphs"), "--out_dir", str(npy_dir), "--resolution", RES, "--save_3d", "--no_save_2d",
                                  "--binarize", "--save_3d_as", ".npy"])
    for path in files:
        name = os.path.basename(path)[:-4]
        want, _ = tree2img.voxelize_forest(_forest(path), [48, 48, 13])
        assert np.array_equal(nifti.read(str(raw_dir / (name + "_3d.nii.gz")))[0], want)
        got = np.load(str(npy_dir / (name + "_3d_label.npy")))
        assert got.dtype == np.bool_ and np.array_equal(got, want >= 1)


def _cut_down_config(base, volumes, out):
    with open(os.path.join(ROOT, "configs", "config_3d_recon_supervised.yml")) as f:
        cfg = yaml.safe_load(f)
    cfg["General"]["model"]["out_channels"] = 4
    cfg["General"]["seed"] = 5
    assert cfg["General"]["amp"] is True
    tr = cfg["Train"]
    tr["data"] = {"image": {"files": str(base / "graphs" / "**" / "*.csv")}, "label": {"files": str(volumes / "*_3d_label.nii.gz")}}
    tr.update(epochs=1, epochs_decay=0, batch_size=1, save_interval=1)                 # two graphs: one epoch of two steps
    for d in tr["data_augmentation"]:
        if d["name"] == "LoadGraphAndFilterByRandomRadiusd":
            d["image_resolutions"] = [[48, 48]]
        if d["name"] == "SelectSlice":
            assert d["slice_selection"] == [[5, -4]]
    cfg["Test"]["data"] = {"image": {"files": str(base / "images" / "*.png")}}
    cfg["Output"]["save_dir"] = str(out)
    return cfg


def test_train_and_test_clis_on_the_cut_down_config(graphs, volumes, tmp_path):
    """train.py: one epoch of two steps with out_channels 4 and amp under OCTA_STRICT=1 -> finite loss in metrics.csv, a checkpoint.
    test.py on that checkpoint in fp32 -> <inference>_<name>.nii.gz, a uint8 volume (48, 48, 4) of 0 / 255. The prefix is the network
    name test.py resolves General.inference to (`model`; `pred` only when nothing resolves it, tests/test_training_cli.py)."""
    import test as test_cli
    import train as train_cli
    import visualize_vessel_graphs
    from octa_autosegmentation_amd import nifti
    from octa_autosegmentation_amd.models import networks
    assert os.environ.get("OCTA_STRICT") == "1"
    base, files = graphs
    # en-face images of the same graphs for test.py
    visualize_vessel_graphs.main(["--source_dir", str(base / "graphs"), "--out_dir", str(base / "images"), "--resolution", RES])
    cfg = _cut_down_config(base, volumes, tmp_path / "results")
    cfg_path = str(tmp_path / "cfg.yml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(cfg, f)
    vendor0 = networks.PATH_COUNTS["vendor"]
    run = train_cli.main(["--config_file", cfg_path, "--num_workers", "0"])
    assert networks.PATH_COUNTS["vendor"] == vendor0
    rows = open(os.path.join(run, "metrics.csv")).read().splitlines()
    assert rows[0].startswith("epoch,train_DiceBCELoss") and len(rows) == 2
    vals = dict(zip(rows[0].split(","), (float(v) for v in rows[1].split(","))))
    print("metrics.csv:", vals)
    assert np.isfinite(vals["train_DiceBCELoss"]) and 0 < vals["train_DiceBCELoss"] < 2
    assert os.path.isfile(os.path.join(run, "checkpoints", "latest_model_model.pth"))

    test_cfg = copy.deepcopy(cfg)
    test_cfg["Output"]["save_dir"] = run
    test_cfg["Test"]["save_dir"] = str(tmp_path / "predictions")
    test_cfg_path = str(tmp_path / "test_cfg.yml")
    with open(test_cfg_path, "w") as f:
        yaml.safe_dump(test_cfg, f)
    written = test_cli.main(["--config_file", test_cfg_path, "--epoch", "latest", "--num_workers", "0"])
    names = sorted(os.path.basename(p)[:-4] for p in files)
    assert sorted(os.path.basename(w) for w in written) == [f"model_{n}.nii.gz" for n in names]
    for w in written:
        vol, hdr = nifti.read(w)
        assert vol.dtype == np.uint8 and vol.shape == (48, 48, 4) and hdr["datatype"] == 2 and set(np.unique(vol)) <= {0, 255}
