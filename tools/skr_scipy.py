"""tools/skr_scipy.py -- a stand-in for the absent scikit-image's `skimage.morphology.area_opening` / `area_closing`, for
tools/make_golden_skrgan.py and tools/time_skrgan.py: the sorted union-find (max-tree) restatement of tests/_morph_ref.py behind
scikit-image's signatures. From a recollection of scikit-image's source, NOT pinned against it: the closing runs the opening on
`invert(image)` = 1 - image for a float image and inverts the result, and an image of fewer pixels than the threshold gives 0
everywhere. The opening is asserted equal to the brute-force definition on small planes by `self_check()`."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

from _morph_ref import brute_opening, uf_opening  # noqa: E402


def area_opening(image, area_threshold=64, connectivity=1, parent=None, tree_traverser=None):
    assert connectivity == 1 and parent is None and tree_traverser is None and image.ndim == 2
    if image.size < area_threshold:
        return np.zeros_like(image)
    if np.isnan(image).any():           # no order to speak of: the caller's constant image after 0 / 0
        return image.copy()
    return uf_opening(image, int(area_threshold))


def area_closing(image, area_threshold=64, connectivity=1, parent=None, tree_traverser=None):
    assert image.dtype == np.float32
    one = np.float32(1)
    return one - area_opening(one - image, area_threshold, connectivity, parent, tree_traverser)


def self_check():
    rng = np.random.default_rng(7)
    n = 0
    for trial in range(24):
        h, w = (int(v) for v in rng.integers(3, 13, 2))
        f = rng.random((h, w)) if trial % 3 == 0 else rng.integers(0, 3 if trial % 3 == 1 else 6, (h, w)) / 5
        f = f.astype(np.float32)
        for lam in (1, 2, 5, 17, 64):
            if f.size >= lam:
                assert np.array_equal(area_opening(f, lam), brute_opening(f, lam)), (trial, lam)
                n += 1
    return n


if __name__ == "__main__":
    print("area opening equals the definition on", self_check(), "planes")
