"""CPU: the 2-D skeleton of the clDice metric (utils/skeleton.py skeletonize_host) against a literal per-pixel oracle written here
from Zhang & Suen's published rule and against known answers, ClDiceMetric against the reference's own scores
(tests/golden/cldice_golden.npz, tools/make_golden_cldice.py), and the validation phase's metric columns.

Parity with scikit-image itself is unpinned (it is not installed): the oracle, the rule's table sizes and the known answers pin it."""
import functools
import os

import numpy as np
import pytest
import torch

from octa_autosegmentation_amd.utils.skeleton import removal_tables, skeletonize_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def oracle(mask):
    """Zhang & Suen 1984, literally: (skeleton, number of double passes that removed something). No table, no code of the package."""
    img = [[1 if v else 0 for v in row] for row in np.asarray(mask).tolist()]
    h, w = len(img), len(img[0])
    at = lambda im, y, x: im[y][x] if 0 <= y < h and 0 <= x < w else 0
    fg = [(y, x) for y in range(h) for x in range(w) if img[y][x]]
    removing = 0
    while True:
        removed = False
        for sub in (1, 2):
            gone = []                                     # decided on the image as it is when the sub-iteration begins, removed at once after it
            for y, x in fg:
                p2, p3, p4, p5 = at(img, y - 1, x), at(img, y - 1, x + 1), at(img, y, x + 1), at(img, y + 1, x + 1)
                p6, p7, p8, p9 = at(img, y + 1, x), at(img, y + 1, x - 1), at(img, y, x - 1), at(img, y - 1, x - 1)
                seq = [p2, p3, p4, p5, p6, p7, p8, p9, p2]
                b = sum(seq[:8])
                a = sum(1 for i in range(8) if seq[i] == 0 and seq[i + 1] == 1)
                if not (2 <= b <= 6 and a == 1):
                    continue
                if sub == 1 and p2 * p4 * p6 == 0 and p4 * p6 * p8 == 0:
                    gone.append((y, x))
                if sub == 2 and p2 * p4 * p8 == 0 and p2 * p6 * p8 == 0:
                    gone.append((y, x))
            for y, x in gone:
                img[y][x] = 0
            if gone:
                removed = True
                fg = [(y, x) for y, x in fg if img[y][x]]
        if not removed:
            return np.array(img, dtype=np.uint8).reshape(h, w), removing
        removing += 1


def random_mask(shape, density, seed=0):
    return (np.random.default_rng([seed, shape[0], shape[1], int(density * 100)]).random(shape) < density).astype(np.uint8)


def disc():
    y, x = np.ogrid[0:200, 0:200]
    return ((y - 100) ** 2 + (x - 100) ** 2 < 90 ** 2).astype(np.uint8)


def recalled_ellipse():
    X, Y = np.ogrid[0:9, 0:9]
    return (1 / 3 * (X - 4) ** 2 + (Y - 4) ** 2 < 9).astype(np.uint8)


def _pixels(shape, coords):
    out = np.zeros(shape, dtype=np.uint8)
    for y, x in coords:
        out[y, x] = 1
    return out


# name -> (input, expected skeleton or None, expected pixel count or None)
KNOWN = {
    "1x1": (np.ones((1, 1), np.uint8), np.ones((1, 1), np.uint8), 1),
    "1x6": (np.ones((1, 6), np.uint8), np.ones((1, 6), np.uint8), 6),
    "2x2": (np.ones((2, 2), np.uint8), np.zeros((2, 2), np.uint8), 0),                 # Zhang-Suen erases it
    "3x7": (np.ones((3, 7), np.uint8), _pixels((3, 7), [(1, 1), (1, 2), (1, 3), (1, 4)]), 4),
    "5x5": (np.ones((5, 5), np.uint8), _pixels((5, 5), [(2, 2)]), 1),
    "8x8": (np.ones((8, 8), np.uint8), _pixels((8, 8), [(3, 3)]), 1),
    "full97x131": (np.ones((97, 131), np.uint8), None, 34),
    "disc": (disc(), None, 1),
    # scikit-image's documented example AS THE MAINTAINER RECALLS IT -- recalled documentation, not a run of scikit-image
    "recalled_ellipse": (recalled_ellipse(), _pixels((9, 9), [(3, 4), (4, 4), (5, 4)]), 3),
}


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """Oracle results, computed once and shared (also with tests/test_skeleton_gpu.py); callers must not write into them."""
    if name in KNOWN:
        res = oracle(KNOWN[name][0])
    else:
        kind, h, w, d = name.split("_")
        res = oracle(random_mask((int(h), int(w)), int(d) / 100))
    res[0].setflags(write=False)
    return res


def test_rule_tables():
    first, second = removal_tables()
    assert int(first.sum()) == 34 and int(second.sum()) == 34 and int((first & second).sum()) == 28


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(name):
    mask, expect, count = KNOWN[name]
    got, removing = skeletonize_host(mask, return_passes=True)
    assert got.dtype == np.uint8 and got.shape == mask.shape and int(got.sum()) == count
    if expect is not None:
        assert np.array_equal(got, expect)
    ref, ref_removing = oracle_of(name)
    assert np.array_equal(got, ref) and removing == ref_removing
    if name == "full97x131":
        assert removing == 48 and removing > 32           # more than a few chunks of a chunked termination loop
    if name == "disc":
        assert removing == 64


@pytest.mark.parametrize("density", [35, 50, 62])
def test_random_masks_equal_the_literal_oracle(density):
    mask = random_mask((97, 131), density / 100)
    ref, ref_removing = oracle_of(f"random_97_131_{density}")
    got, removing = skeletonize_host(mask, return_passes=True)
    assert np.array_equal(got, ref) and removing == ref_removing
    assert 0 < got.sum() < mask.sum()


def test_host_input_forms():
    mask = random_mask((20, 33), 0.5)
    ref = skeletonize_host(mask)
    assert np.array_equal(skeletonize_host(mask.astype(bool)), ref)
    assert np.array_equal(skeletonize_host(mask * np.float32(-0.25)), ref)            # non-zero is foreground
    assert np.array_equal(skeletonize_host(np.asfortranarray(mask * 7)), ref)
    assert mask.sum() > ref.sum()                                                      # and the input is left alone
    with pytest.raises(NotImplementedError):
        skeletonize_host(np.ones((3, 4, 5)))


def packed_word_emulation(mask):
    """The kernel's scheme (csrc/skeleton.hip) restated on python integers, word by word: 64 pixels per word, bit i = pixel 64 xw + i,
    neighbour planes from one-bit shifts plus the carry bit of the adjacent word, B as a bit-sliced counter, A as "at least one step and
    not at least two", two buffers per double pass. Returns (skeleton, removing double passes)."""
    full = (1 << 64) - 1
    h, w = mask.shape
    wq = (w + 63) // 64
    a = [[sum(1 << (x & 63) for x in range(64 * xw, min(w, 64 * xw + 64)) if mask[y, x]) for xw in range(wq)] for y in range(h)]

    def sub(src, second):
        at = lambda y, xw: src[y][xw] if 0 <= y < h and 0 <= xw < wq else 0
        dst, flag = [[0] * wq for _ in range(h)], False
        for y in range(h):
            for xw in range(wq):
                c = src[y][xw]
                if not c:
                    continue
                n, s = at(y - 1, xw), at(y + 1, xw)
                east = lambda word, right: (word >> 1) | ((right << 63) & full)
                west = lambda word, left: ((word << 1) & full) | (left >> 63)
                p = [n, east(n, at(y - 1, xw + 1)), east(c, at(y, xw + 1)), east(s, at(y + 1, xw + 1)),
                     s, west(s, at(y + 1, xw - 1)), west(c, at(y, xw - 1)), west(n, at(y - 1, xw - 1))]
                b0 = b1 = b2 = b3 = one = two = 0
                for k in range(8):
                    q = p[k]
                    c0 = b0 & q
                    b0 ^= q
                    c1 = b1 & c0
                    b1 ^= c0
                    c2 = b2 & c1
                    b2 ^= c1
                    b3 |= c2
                    step = ~q & full & p[(k + 1) & 7]
                    two |= one & step
                    one |= step
                ok = ~b3 & (b1 | b2) & ~(b0 & b1 & b2) & one & ~two & full
                p2, p4, p6, p8 = p[0], p[2], p[4], p[6]
                cond = (~(p2 & p4 & p8) & ~(p2 & p6 & p8)) if second else (~(p2 & p4 & p6) & ~(p4 & p6 & p8))
                gone = c & ok & cond & full
                flag = flag or gone != 0
                dst[y][xw] = c & ~gone & full
        return dst, flag

    removing = 0
    while True:
        b, f1 = sub(a, False)
        a, f2 = sub(b, True)
        if not (f1 or f2):
            break
        removing += 1
    return np.array([[(a[y][x >> 6] >> (x & 63)) & 1 for x in range(w)] for y in range(h)], dtype=np.uint8).reshape(h, w), removing


@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (9, 9), (33, 64), (21, 65), (20, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_packed_word_scheme_equals_host(shape):
    """The bit-packed formulation the kernel uses, without a GPU: word seams at 64 and 128, widths that are no multiple of the word."""
    for density in (0.5, 0.62, 1.0):
        mask = random_mask(shape, density, seed=1)
        ref, removing = skeletonize_host(mask, return_passes=True)
        got, n = packed_word_emulation(mask)
        assert np.array_equal(got, ref) and n == removing, (shape, density)


def load_golden():
    z = np.load(os.path.join(GOLDEN, "cldice_golden.npz"))
    return [(str(n), z[f"{n}_pred"], z[f"{n}_label"], z[f"{n}_scores"]) for n in z["names"]], float(z["aggregate"])


def check_metric_against_golden(device):
    """ClDiceMetric on `device` against the reference's recorded scores: 1e-12 per score, NaN where recorded, and the nanmean aggregate
    (this project's Metric.aggregate hands a float32 on: the recorded float64 rounded to float32, exactly)."""
    from octa_autosegmentation_amd.utils.metrics import ClDiceMetric
    cases, aggregate = load_golden()
    assert {"emptypred", "emptylabel", "disjoint", "softpred", "twolayer"} <= {c[0] for c in cases}
    metric = ClDiceMetric()
    n = 0
    for name, pred, label, scores in cases:
        metric([torch.from_numpy(pred).to(device)], [torch.from_numpy(label).to(device)])
        got = metric.scores[n:]
        n += len(scores)
        assert len(got) == len(scores), name
        for g, s in zip(got, scores):
            assert g.dim() == 0 and g.device.type == torch.device(device).type, name
            g = float(g)
            assert (np.isnan(g) and np.isnan(s)) or abs(g - s) <= 1e-12, (name, g, s)
    assert sum(int(np.isnan(c[3]).sum()) for c in cases) == 4
    got = metric.aggregate()
    assert got.dtype == torch.float32 and float(got) == float(np.float32(aggregate))


def test_cldice_metric_matches_reference_scores():
    check_metric_against_golden("cpu")


def test_validation_metric_columns_in_reference_order():
    from octa_autosegmentation_amd.utils.enums import Phase
    from octa_autosegmentation_amd.utils.metrics import MetricsManager
    assert list(MetricsManager(Phase.VALIDATION).metrics) == ["DSC", "IoU", "ClDice", "AUC", "ACC", "Recall", "Precision"]
    assert list(MetricsManager(Phase.TRAIN).metrics) == ["DSC", "IoU"]
    import octa_autosegmentation_amd.utils.metrics as m
    assert not hasattr(m, "_have_skimage")


def test_three_dimensional_layers_are_refused():
    from octa_autosegmentation_amd.utils.metrics import ClDiceMetric
    vol = torch.ones(1, 4, 8, 8)
    with pytest.raises(NotImplementedError, match="lee"):
        ClDiceMetric()([vol], [vol])
