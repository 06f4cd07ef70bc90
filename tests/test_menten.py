"""CPU: the Menten et al. augmentation (MentenAugmentationd = BinomialVesselNoised -> AddVitreousFloater -> AddMotionArtifact, reference
data/data_transforms.py:44-325) -- registry, the host restatement against the reference's own outputs (tests/golden/menten_golden.npz,
tools/make_golden_menten.py) bit for bit including dtypes and the position of numpy's global stream afterwards, the Bresenham
restatement of skimage.draw.line against hand-written point lists, and the per-row gather table the motion kernel is driven by."""
import numpy as np
import pytest
import torch

import _menten_cases as C
from octa_autosegmentation_amd.data import data_transforms as T
from octa_autosegmentation_amd.data import menten

CPU = torch.device("cpu")


def same(t, want):
    a = t.numpy()
    return a.dtype == want.dtype and a.shape == want.shape and np.array_equal(a, want)


def test_registry_builds_the_four_transforms_and_declares_numpy_stream():
    cfg = [{"name": "BinomialVesselNoised", "keys": ["image"], "r": 20},
           {"name": "AddVitreousFloater", "keys": ["image"], "floater_chance": 0.5},
           {"name": "AddMotionArtifact", "img_key": "image", "gt_key": "label", "max_shear": 3},
           {"name": "MentenAugmentationd", "img_key": "image", "gt_key": "label"}]
    ts = T.get_data_augmentations(cfg, seed=1)
    assert [type(t).__name__ for t in ts] == [d["name"] for d in cfg]
    assert ts[0].r == 20 and ts[0].vessel_noise_scaling == 0.5 and ts[0].vessel_noise_blur == 1.0
    assert ts[1].floater_chance == 0.5 and tuple(ts[1].dilations_interval) == (10, 30) and tuple(ts[1].floater_segments_interval) == (10, 20)
    assert ts[2].max_shear == 3 and ts[2].grace_margin == 10 and ts[2].no_h_cuts == 3 and ts[2].keys == ["image", "label"]
    assert ts[3].binomialVesselNoised.r == 48 and ts[3].vitreousFloater.floater_chance == 0.1
    for t in ts:
        assert t.rng_streams() == {"numpy"} and t.rng_streams(has_background=False) == {"numpy"}
    # behind the frozen generator's cut a chain with numpy draws on both sides must not be batched
    chain = T.Compose([T.AddRandomBackgroundNoised(["image"]), type("Cut", (), {"batch_apply": None})(), ts[3]])
    assert not chain.batchable()


@pytest.mark.parametrize("k", C.vessel_cases())
def test_vessel_noise_host_path_is_the_reference_bit_for_bit(k):
    g = C.golden()
    out, nxt, x, keep = C.run_vessel(k, CPU)
    assert same(out, g[f"vessel_{k}_out"]) and out.dtype == torch.float64
    assert nxt == float(g[f"vessel_{k}_next"])
    assert torch.equal(x, keep)


def test_vessel_case_has_a_pixel_exactly_on_a_ring():
    h = 64
    assert np.sqrt((32 + 12 - h / 2) ** 2 + (32 + 16 - h / 2) ** 2) == 20.0 == C.golden()["vessel_0_args"][2]


@pytest.mark.parametrize("k", C.floater_cases())
def test_floater_host_path_is_the_reference_bit_for_bit(k):
    g = C.golden()
    out, nxt, x, keep = C.run_floater(k, CPU)
    assert same(out, g[f"floater_{k}_out"])
    assert nxt == float(g[f"floater_{k}_next"])
    assert torch.equal(x, keep)
    if k == 3:          # default chance, no floater: the image comes back untouched in its own dtype
        assert out.dtype == torch.float32 and torch.equal(out, keep)
    else:
        assert out.dtype == torch.float64 and not np.array_equal(out.numpy(), g[f"floater_{k}_in"])


def test_floater_fixture_walks():
    """The cases are what they are meant to be: case 0 stays inside, case 2 leaves the image, case 1 is smaller than the blur radius."""
    g = C.golden()
    walks = {}
    for k in (0, 1, 2):
        np.random.seed(int(g[f"floater_{k}_seed"]))
        n = g[f"floater_{k}_in"].shape[-1]
        pts = menten.floater_draws(n, n, 1.0)[0]
        walks[k] = bool(np.all((pts >= 0) & (pts < n)))
    assert walks[0] and not walks[2]
    assert g["floater_1_in"].shape[-1] < menten.gaussian_radius(10) == 40


def test_floater_on_a_non_square_image_raises_like_the_reference():
    g = C.golden()
    x = torch.from_numpy(g["floater_4_in"].copy())
    np.random.seed(int(g["floater_4_seed"]))
    with pytest.raises(ValueError, match="could not be broadcast"):
        T.AddVitreousFloater(["image"], floater_chance=1.0)({"image": x})
    assert np.random.uniform() == float(g["floater_4_next"])            # the draws were made before it raised


@pytest.mark.parametrize("seed", C.motion_seeds())
def test_motion_host_path_is_the_reference_bit_for_bit(seed):
    g = C.golden()
    img, gt, nxt, (x, y), (kx, ky) = C.run_motion(seed, CPU)
    assert same(img, g[f"motion_{seed}_out"]) and img.dtype == torch.float64
    assert same(gt, g[f"motion_{seed}_gt"]) and gt.dtype == torch.float32
    assert nxt == float(g[f"motion_{seed}_next"])
    assert torch.equal(x, kx) and torch.equal(y, ky)
    assert img.data_ptr() != x.data_ptr() and gt.data_ptr() != y.data_ptr()        # new tensors, also for zero cuts


def test_motion_fixture_covers_every_kind():
    g = C.golden()
    cuts = {s: [c.split(":") for c in g[f"motion_{s}_kinds"]] for s in C.motion_seeds()}
    kinds = {k for c in cuts.values() for k, _, _ in c}
    assert kinds == {"shear", "stretch", "buckle", "whiteout"}
    assert any(len(c) == 0 for c in cuts.values()) and any(len(c) == 2 for c in cuts.values())
    assert any(k == "shear" and a == "0" for c in cuts.values() for k, _, a in c)


@pytest.mark.parametrize("seed", C.motion_seeds())
def test_motion_gather_table_reproduces_the_reference(seed):
    """menten.fold_cuts (what the motion kernel is driven by), applied with numpy: out[R][j] = 0 for j < shift else source[j - shift]."""
    g = C.golden()

    def gather(x, table, white):
        out = np.zeros_like(x)
        for R, (src, sh) in enumerate(table):
            row = x[src] if src >= 0 else white[-src - 1].astype(x.dtype)
            out[R, sh:] = row[:x.shape[1] - sh]
        return out

    np.random.seed(seed)
    cuts = menten.motion_draws(48, 48, {'shear': 0.3, 'stretch': 0.3, 'buckle': 0.3, 'whiteout': 0.1})
    table, white = menten.fold_cuts(48, 48, cuts, 1)
    assert table.dtype == np.int32 and table.shape == (48, 2)
    assert np.array_equal(gather(g["motion_in"][0], table, white), g[f"motion_{seed}_out"][0])
    table4, white4 = menten.fold_cuts(48, 48, cuts, 4)
    assert white4 is None and table4.shape == (192, 2) and (table4[:, 1] % 4 == 0).all()
    assert np.array_equal(gather(g["motion_gt"][0], table4, None), g[f"motion_{seed}_gt"][0])


def test_menten_chain_host_path_is_the_reference_bit_for_bit():
    g = C.golden()
    img, gt, nxt = C.run_menten(CPU)
    assert same(img, g["menten_out"]) and same(gt, g["menten_gt"]) and nxt == float(g["menten_next"])
    assert img.dtype == torch.float64 and gt.dtype == torch.float32


def test_gaussian_weights_are_scipys():
    from scipy.ndimage import correlate1d, gaussian_filter1d
    x = np.zeros(201)
    x[100] = 1.0
    for sigma in (1.0, 1.5, 10):
        w = menten.gaussian_weights(sigma)
        r = menten.gaussian_radius(sigma)
        assert len(w) == 2 * r + 1
        assert np.array_equal(gaussian_filter1d(x, sigma)[100 - r:100 + r + 1], correlate1d(x, w)[100 - r:100 + r + 1])
        assert np.array_equal(gaussian_filter1d(x, sigma)[100 - r:100 + r + 1], w[::-1])


LINES = {
    # octants, from (0, 0): dc > dr and dr > dc with every sign combination
    (0, 0, 2, 5): [(0, 0), (0, 1), (1, 2), (1, 3), (2, 4), (2, 5)],
    (0, 0, 5, 2): [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2)],
    (0, 0, 5, -2): [(0, 0), (1, 0), (2, -1), (3, -1), (4, -2), (5, -2)],
    (0, 0, 2, -5): [(0, 0), (0, -1), (1, -2), (1, -3), (2, -4), (2, -5)],
    (0, 0, -2, -5): [(0, 0), (0, -1), (-1, -2), (-1, -3), (-2, -4), (-2, -5)],
    (0, 0, -5, -2): [(0, 0), (-1, 0), (-2, -1), (-3, -1), (-4, -2), (-5, -2)],
    (0, 0, -5, 2): [(0, 0), (-1, 0), (-2, 1), (-3, 1), (-4, 2), (-5, 2)],
    (0, 0, -2, 5): [(0, 0), (0, 1), (-1, 2), (-1, 3), (-2, 4), (-2, 5)],
    # a single point, horizontal, vertical, the two diagonals
    (3, 4, 3, 4): [(3, 4)],
    (1, 1, 1, 4): [(1, 1), (1, 2), (1, 3), (1, 4)],
    (1, 4, 1, 1): [(1, 4), (1, 3), (1, 2), (1, 1)],
    (4, 2, 1, 2): [(4, 2), (3, 2), (2, 2), (1, 2)],
    (0, 0, 3, 3): [(0, 0), (1, 1), (2, 2), (3, 3)],
    (3, 0, 0, 3): [(3, 0), (2, 1), (1, 2), (0, 3)],
}


@pytest.mark.parametrize("ends", sorted(LINES))
def test_bresenham_against_hand_written_point_lists(ends):
    rr, cc = menten.draw_line(*ends)
    assert list(zip(rr.tolist(), cc.tolist())) == LINES[ends]
    assert len(rr) == max(abs(ends[2] - ends[0]), abs(ends[3] - ends[1])) + 1
