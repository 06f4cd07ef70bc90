"""References for the 3-D connected-component filter (csrc/cc3d.hip): scipy.ndimage.label + bincount, a literal numpy restatement of
the reference's RemoveOuterNoise (data/data_transforms.py:418-432), and a breadth-first flood fill that uses no scipy."""
from collections import deque
from itertools import product

import numpy as np
from scipy import ndimage

DENSITY = {3: 0.10, 2: 0.14, 1: 0.31}       # near each neighbourhood's site-percolation threshold: components of every size


def label(mask, connectivity):
    """Raster-ordered labels (1 .. n in the C order of each component's first voxel) of a 3-D mask; connectivity 1 / 2 / 3 = 6 / 18 / 26."""
    return ndimage.label(np.asarray(mask) != 0, structure=ndimage.generate_binary_structure(3, connectivity))


def info(mask, connectivity):
    """(number of components, voxels of the largest, flat index of its first voxel or -1)."""
    lab, n = label(mask, connectivity)
    if n == 0:
        return 0, 0, -1
    counts = np.bincount(lab.ravel())
    best = int(np.argmax(counts[1:])) + 1
    return n, int(counts[best]), int(np.flatnonzero(lab.ravel() == best)[0])


def keep_largest(mask, connectivity):
    """uint8 0 / 1: the component with the most voxels; "largest" is argmax(counts[1:]) + 1, so a tie goes to the lowest label."""
    lab, n = label(mask, connectivity)
    if n == 0:
        return np.zeros(lab.shape, np.uint8)
    return (lab == int(np.argmax(np.bincount(lab.ravel())[1:])) + 1).astype(np.uint8)


def remove_small(mask, min_size, connectivity):
    """uint8 0 / 1: the components with at least min_size voxels."""
    lab, _ = label(mask, connectivity)
    counts = np.bincount(lab.ravel())
    keep = counts >= min_size
    keep[0] = False
    return keep[lab].astype(np.uint8)


def remove_outer_noise(volume, z_axis=0):
    """The reference's RemoveOuterNoise.__call__, line by line, on numpy."""
    volume_tmp = np.array(volume).astype(bool)[None]
    volume_tmp[0, volume.shape[z_axis] // 2] = True
    volume_tmp = keep_largest(volume_tmp[0], 3).astype(bool)
    return np.logical_and(volume, volume_tmp)


def flood_keep_largest(mask, connectivity):
    """keep_largest by breadth-first flood fill in raster order of the seeds, without scipy."""
    mask = np.asarray(mask) != 0
    offs = [o for o in product((-1, 0, 1), repeat=3) if 0 < sum(map(abs, o)) <= connectivity]
    seen, best = np.zeros(mask.shape, bool), []
    for seed in zip(*np.nonzero(mask)):
        if seen[seed]:
            continue
        seen[seed], comp, queue = True, [seed], deque([seed])
        while queue:
            z, y, x = queue.popleft()
            for dz, dy, dx in offs:
                n = (z + dz, y + dy, x + dx)
                if all(0 <= c < s for c, s in zip(n, mask.shape)) and mask[n] and not seen[n]:
                    seen[n] = True
                    comp.append(n)
                    queue.append(n)
        if len(comp) > len(best):           # strictly more: the first of equals stays
            best = comp
    out = np.zeros(mask.shape, np.uint8)
    for n in best:
        out[n] = 1
    return out


def random_mask(shape, density, seed, fill_plane=False):
    m = (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)
    if fill_plane:
        m[shape[0] // 2] = 1
    return m


PINNED = {(9, 70, 67): (475, 7583), (44, 96, 80): (4484, 22877), (44, 304, 304): (72557, 145646)}     # components, voxels of the largest (scipy, 26)


def pinned_volumes():
    """Three thresholded random fields with the central plane filled, drawn one after the other from default_rng(3): 9 x 70 x 67 and
    44 x 96 x 80 at 10 %, 44 x 304 x 304 at 8 %. What scipy finds in them at connectivity 3 is PINNED (the second largest component of
    the first has 14 voxels)."""
    rng, out = np.random.default_rng(3), {}
    for shape, density in (((9, 70, 67), 0.10), ((44, 96, 80), 0.10), ((44, 304, 304), 0.08)):
        m = (rng.random(shape) < density).astype(np.uint8)
        m[shape[0] // 2] = 1
        out[shape] = m
    return out


def serpentine(shape=(12, 40, 200)):
    """One 6-connected path, one voxel wide, through every second row of every second plane: it visits every 4 x 8 x 64 brick."""
    D, H, W = shape
    m = np.zeros(shape, np.uint8)
    rows = list(range(0, H, 2))
    assert len(rows) % 2 == 0                  # the path through a plane starts and ends at x = 0
    for zi, z in enumerate(range(0, D, 2)):
        for yi, y in enumerate(rows):
            m[z, y, :] = 1
            if yi + 1 < len(rows):
                m[z, y + 1, W - 1 if yi % 2 == 0 else 0] = 1
        if z + 2 < D:
            m[z + 1, rows[-1] if zi % 2 == 0 else 0, 0] = 1
    return m


def two_bars():
    """Two 3-voxel bars at opposite corners of a 3 x 5 x 9 volume: a tie, the one at the origin wins."""
    m = np.zeros((3, 5, 9), np.uint8)
    m[0, 0, :3] = 1
    m[2, 4, 6:] = 1
    return m
