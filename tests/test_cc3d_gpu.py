"""GPU: the 3-D connected-component filter (csrc/cc3d.hip) byte for byte against scipy.ndimage.label + bincount (tests/_cc3d_ref.py):
shapes that put components across every kind of brick seam, ties, empty and full volumes, batches, long components through many bricks,
one mid-size volume, sentinels, repeatability, the transforms built on it, and test.py on the cut-down 3-D config with RemoveOuterNoise."""
import copy
import glob
import os

import numpy as np
import pytest
import yaml

import _cc3d_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_SIZE = 20
SEAM_SHAPES = [(9, 70, 67), (44, 96, 80), (1, 97, 131), (5, 1, 300), (3, 130, 1)]


def _run(masks, connectivity, mode, min_size=MIN_SIZE):
    """masks: numpy [B,D,H,W] -> (out numpy uint8 [B,D,H,W], info numpy int64 [B,3])."""
    import torch
    from octa_autosegmentation_amd.models import postprocess
    out, info = postprocess.cc3d_filter_device(torch.from_numpy(np.ascontiguousarray(masks)).cuda(), connectivity, mode, min_size, return_info=True)
    return out.cpu().numpy(), info.cpu().numpy()


def _check(masks, connectivity):
    """Both modes and d_info of a batch against the reference, volume by volume."""
    masks = np.asarray(masks)
    small, info0 = _run(masks, connectivity, 0)
    largest, info1 = _run(masks, connectivity, 1)
    for b, m in enumerate(masks):
        want = ref.info(m, connectivity)
        assert tuple(info0[b]) == want and tuple(info1[b]) == want, (b, info0[b], info1[b], want)
        assert np.array_equal(small[b], ref.remove_small(m, MIN_SIZE, connectivity)), b
        assert np.array_equal(largest[b], ref.keep_largest(m, connectivity)), b


@pytest.fixture(scope="module")
def pinned():
    return ref.pinned_volumes()


@pytest.mark.parametrize("connectivity", [1, 2, 3])
def test_seam_shapes(hip_lib_built, pinned, connectivity):
    for i, shape in enumerate(SEAM_SHAPES):
        _check(ref.random_mask(shape, ref.DENSITY[connectivity], 100 + 10 * connectivity + i)[None], connectivity)
        _check(ref.random_mask(shape, ref.DENSITY[connectivity], 200 + 10 * connectivity + i, fill_plane=True)[None], connectivity)
    for shape in ((9, 70, 67), (44, 96, 80)):          # the pinned fields: 475 components / 7 583 voxels, 4 484 / 22 877 at connectivity 3
        _check(pinned[shape][None], connectivity)
    if connectivity == 3:
        for shape in ((9, 70, 67), (44, 96, 80)):
            assert tuple(_run(pinned[shape][None], 3, 1)[1][0][:2]) == ref.PINNED[shape]
    d = ref.DENSITY[connectivity]
    _check(np.stack([ref.random_mask((13, 17, 129), f * d, 300 + connectivity + j) for j, f in enumerate((0.6, 1.0, 1.5))]), connectivity)


@pytest.mark.parametrize("connectivity", [1, 2, 3])
def test_ties_empty_full_and_batch_boundary(hip_lib_built, connectivity):
    bars = ref.two_bars()
    out, info = _run(bars[None], connectivity, 1)
    want = np.zeros_like(bars)
    want[0, 0, :3] = 1
    assert np.array_equal(out[0], want) and tuple(info[0]) == (2, 3, 0)
    _check(bars[None], connectivity)
    for shape in ((3, 5, 9), (5, 9, 70)):
        empty, full = np.zeros(shape, np.uint8), np.ones(shape, np.uint8)
        for mode in (0, 1):
            out, info = _run(np.stack([empty, full]), connectivity, mode)
            assert not out[0].any() and tuple(info[0]) == (0, 0, -1)
            assert out[1].all() == (mode == 1 or full.size >= MIN_SIZE) and tuple(info[1]) == (1, full.size, 0)
    # volume 0 ends with a filled plane, volume 1 starts with one: two components of equal size if -- and only if -- volumes stay apart
    pair = np.zeros((2, 5, 9, 70), np.uint8)
    pair[0, -1], pair[1, 0] = 1, 1
    pair[0, 0, 0, :3] = 1
    out, info = _run(pair, connectivity, 1)
    assert np.array_equal(out[0], (np.arange(5) == 4)[:, None, None] * np.ones((5, 9, 70), np.uint8)) and tuple(info[0]) == (2, 630, 4 * 630)
    assert np.array_equal(out[1], pair[1]) and tuple(info[1]) == (1, 630, 0)
    _check(pair, connectivity)


def test_long_components_across_many_bricks(hip_lib_built):
    s = ref.serpentine()
    s[11, 39, 199] = 1                                   # and one speck
    out, info = _run(s[None], 1, 1)                      # (at connectivity 2 and 3 the speck touches the path diagonally)
    assert tuple(info[0]) == (2, int(s.sum()) - 1, 0) and out[0].sum() == s.sum() - 1 and out[0, 11, 39, 199] == 0
    for connectivity in (1, 2, 3):
        _check(s[None], connectivity)
    z, y, x = np.indices((6, 18, 70))
    board = ((z + y + x) % 2 == 0).astype(np.uint8)
    out, info = _run(board[None], 3, 1)
    assert np.array_equal(out[0], board) and tuple(info[0]) == (1, int(board.sum()), 0)
    out, info = _run(board[None], 1, 1)                  # every voxel its own component: voxel 0 is the first of equals
    assert out[0].sum() == 1 and out[0, 0, 0, 0] == 1 and tuple(info[0]) == (int(board.sum()), 1, 0)
    assert not _run(board[None], 1, 0, min_size=2)[0].any() and np.array_equal(_run(board[None], 1, 0, min_size=1)[0][0], board)
    for connectivity in (1, 2, 3):
        _check(board[None], connectivity)


def test_mid_size_volume_sentinels_and_repeatability(hip_lib_built, pinned):
    import torch
    from octa_autosegmentation_amd import _native
    m = pinned[(44, 304, 304)]
    out, info = _run(m[None], 3, 1)
    assert tuple(info[0][:2]) == ref.PINNED[m.shape] == (72557, 145646) and tuple(info[0]) == ref.info(m, 3)
    assert np.array_equal(out[0], ref.keep_largest(m, 3))
    out0, _ = _run(m[None], 3, 0)
    assert np.array_equal(out0[0], ref.remove_small(m, MIN_SIZE, 3))
    # 64 sentinel bytes on either side of d_out, on an odd shape; on_value other than 1; twice
    for shape, mode in (((9, 70, 67), 0), ((9, 70, 67), 1), ((44, 304, 304), 1)):
        mm = pinned[shape]
        d_in = torch.from_numpy(mm).cuda()
        runs = []
        for _ in range(2):
            buf = torch.full((mm.size + 128,), 0xA5, dtype=torch.uint8, device="cuda")
            d_out = buf[64:64 + mm.size]
            _native.launch("octa_cc3d_filter", d_in.device, d_in, 1, *mm.shape, 3, mode, MIN_SIZE, 255, d_out, None)
            assert (buf[:64] == 0xA5).all() and (buf[-64:] == 0xA5).all()
            runs.append(d_out.clone())
        assert torch.equal(runs[0], runs[1])
        want = ref.keep_largest(mm, 3) if mode else ref.remove_small(mm, MIN_SIZE, 3)
        assert np.array_equal(runs[0].cpu().numpy().reshape(mm.shape), want * 255)


def test_transforms(hip_lib_built, pinned):
    import torch
    from octa_autosegmentation_amd.data import data_transforms as dt
    from octa_autosegmentation_amd.models import postprocess
    v = ref.random_mask((9, 70, 67), 0.10, 7).astype(np.float32)
    x = torch.from_numpy(v).cuda()
    got = dt.RemoveOuterNoise()(x)
    assert got.dtype == torch.bool and got.shape == x.shape and np.array_equal(got.cpu().numpy(), ref.remove_outer_noise(v))
    with pytest.raises(IndexError):
        dt.RemoveOuterNoise(z_axis=1)(x)                 # plane 70 // 2 of dim 0, which has 9
    wide = torch.from_numpy(np.ascontiguousarray(v.transpose(1, 0, 2))).cuda()          # [70, 9, 67]: 9 // 2 = 4 exists in dim 0
    assert np.array_equal(dt.RemoveOuterNoise(z_axis=1)(wide).cpu().numpy(), ref.remove_outer_noise(wide.cpu().numpy(), z_axis=1))
    for shape, conn in (((1, 97, 131), None), ((1, 97, 131), 1), ((1, 9, 70, 67), None), ((1, 9, 70, 67), 2)):
        m = ref.random_mask(shape, 0.2 if len(shape) == 3 else 0.12, 11) * np.float32(3)
        got = dt.KeepLargestConnectedComponent(connectivity=conn)(torch.from_numpy(m).cuda())
        vol = m[0] if len(shape) == 4 else m
        c = conn if conn is not None else len(shape) - 1
        want = (m * ref.keep_largest(vol, c).reshape(m.shape)).astype(np.float32)
        assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want)
    with pytest.raises(NotImplementedError, match="channels"):
        dt.KeepLargestConnectedComponent()(torch.zeros(2, 9, 9, device="cuda"))
    m = ref.random_mask((9, 70, 67), 0.31, 13)
    x = torch.from_numpy(m.astype(np.float32)).cuda()
    got = dt.RemoveSmallObjects(min_size=MIN_SIZE, independent_channels=False)(x)
    assert np.array_equal(got.cpu().numpy(), ref.remove_small(m, MIN_SIZE, 1).astype(np.float32))
    per_slice = np.stack([ref.remove_small(s[None], MIN_SIZE, 1)[0] for s in m]).astype(np.float32)
    assert np.array_equal(dt.RemoveSmallObjects(min_size=MIN_SIZE)(x).cpu().numpy(), per_slice)
    assert torch.equal(dt.RemoveSmallObjects(min_size=MIN_SIZE)(x), x * postprocess.remove_small_objects_device(x, MIN_SIZE).to(x.dtype))
    # the batch form of the YAML list
    logits = torch.from_numpy(np.stack([v, ref.random_mask((9, 70, 67), 0.10, 8)]) * 8 - 4).cuda()
    out = postprocess.postprocess_prediction(logits, [{"name": "Activations", "sigmoid": True}, {"name": "AsDiscrete", "threshold": 0.5},
                                                      {"name": "RemoveOuterNoise"}])
    assert out.dtype == torch.bool and np.array_equal(out[0].cpu().numpy(), ref.remove_outer_noise(v))


# ---- through test.py: the cut-down 3-D config of tests/test_recon3d_gpu.py with RemoveOuterNoise in the test prediction list ----

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
    base = tmp_path_factory.mktemp("cc3d_recon")
    cfg_path = base / "cfg.yml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    out_dir = base / "graphs"
    generate_vessel_graph.main(["--config_file", str(cfg_path), "--num_samples", "2", "--seed", "0", "--output.directory", str(out_dir)])
    files = sorted(glob.glob(str(out_dir / "*" / "*.csv")))
    assert len(files) == 2
    return base, files


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
    cfg["Test"]["data"] = {"image": {"files": str(base / "images" / "*.png")}}
    cfg["Output"]["save_dir"] = str(out)
    return cfg


def test_remove_outer_noise_through_test_cli(graphs, tmp_path):
    """train.py: one epoch of two steps (out_channels 4, 48 x 48) under OCTA_STRICT=1; test.py on that checkpoint twice, without and with
    RemoveOuterNoise between RemoveSmallObjects and AsChannelLast: each model_<name>.nii.gz of the second run is the numpy restatement
    applied to the volume of the first."""
    import test as test_cli
    import train as train_cli
    import visualize_vessel_graphs
    from octa_autosegmentation_amd import nifti
    from octa_autosegmentation_amd.models import networks
    assert os.environ.get("OCTA_STRICT") == "1"
    vendor0 = networks.PATH_COUNTS["vendor"]
    base, files = graphs
    volumes = base / "volumes"
    visualize_vessel_graphs.main(["--source_dir", str(base / "graphs"), "--out_dir", str(volumes), "--resolution", RES, "--save_3d", "--binarize"])
    visualize_vessel_graphs.main(["--source_dir", str(base / "graphs"), "--out_dir", str(base / "images"), "--resolution", RES])
    cfg = _cut_down_config(base, volumes, tmp_path / "results")
    cfg_path = str(tmp_path / "cfg.yml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(cfg, f)
    run = train_cli.main(["--config_file", cfg_path, "--num_workers", "0"])
    written = {}
    for tag in ("plain", "outer"):
        test_cfg = copy.deepcopy(cfg)
        test_cfg["Output"]["save_dir"] = run
        test_cfg["Test"]["save_dir"] = str(tmp_path / ("predictions_" + tag))
        pred = test_cfg["Test"]["post_processing"]["prediction"]
        assert [d["name"] for d in pred] == ["Activations", "AsDiscrete", "RemoveSmallObjects", "AsChannelLast"]
        if tag == "outer":
            pred.insert(3, {"name": "RemoveOuterNoise"})
        path = str(tmp_path / f"test_cfg_{tag}.yml")
        with open(path, "w") as f:
            yaml.safe_dump(test_cfg, f)
        written[tag] = sorted(test_cli.main(["--config_file", path, "--epoch", "latest", "--num_workers", "0"]))
    assert networks.PATH_COUNTS["vendor"] == vendor0
    names = sorted(os.path.basename(p)[:-4] for p in files)
    for tag in written:
        assert [os.path.basename(w) for w in written[tag]] == [f"model_{n}.nii.gz" for n in names]
    for plain, outer in zip(written["plain"], written["outer"]):
        a, _ = nifti.read(plain)
        b, hdr = nifti.read(outer)
        assert b.dtype == np.uint8 and b.shape == (48, 48, 4) and hdr["datatype"] == 2 and set(np.unique(b)) <= {0, 255}
        want = ref.remove_outer_noise(np.moveaxis(a, -1, 0))                      # the transform sees [Z, X, Y]
        assert np.array_equal(b, np.moveaxis(want, 0, -1).astype(np.uint8) * 255)
