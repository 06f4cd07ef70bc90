"""Grey-level area opening / closing on the CPU, three ways, shared by tests/test_skrgan.py, tests/test_skrgan_gpu.py and
tools/skr_scipy.py (the stand-in for the absent scikit-image):

  brute_opening   the definition, level by level: open(f)(p) = max{h <= f(p) : |C_p(h)| >= lam}, C_p(h) the 4-connected component
                  of {f >= h} that contains p (scipy.ndimage.label per level). Small planes only.
  uf_opening      the sorted union-find (max-tree) restatement of Meijster and Wilkinson: pixels in decreasing order, a component
                  is merged into a lower pixel while it is smaller than lam (or of the same value), and frozen otherwise.
  seed_opening    the formulation csrc/morph.hip evaluates, one greedy growth per seed, with the kernel's bookkeeping (the
                  candidates of each region pixel, struck when taken).

The closing is 1 - open(1 - x) with both subtractions in float32 (scikit-image's route through `invert`, as recalled), not the
exact order dual."""
import numpy as np
from scipy import ndimage as ndi


def brute_opening(f, lam):
    f = np.asarray(f)
    assert f.ndim == 2 and f.size >= lam >= 1
    out = np.empty_like(f)
    done = np.zeros(f.shape, bool)
    for h in np.unique(f)[::-1]:                    # the highest level that qualifies wins
        lab, n = ndi.label(f >= h)                  # connectivity 1
        big = np.concatenate([[False], np.bincount(lab.ravel())[1:] >= lam])[lab]
        take = big & ~done
        out[take] = h
        done |= take
    assert done.all()
    return out


def uf_opening(f, lam):
    f = np.asarray(f)
    assert f.ndim == 2 and f.size >= lam >= 1
    h, w = f.shape
    flat = f.ravel()
    vals = flat.tolist()
    order = np.argsort(-flat, kind="stable").tolist()
    n = h * w
    parent = [-2] * n                               # -2: not seen yet, -1: a root
    area = [0] * n
    for p in order:
        parent[p], area[p] = -1, 1
        y, x = divmod(p, w)
        for q in ((p - w) if y > 0 else -1, (p + w) if y < h - 1 else -1, (p - 1) if x > 0 else -1, (p + 1) if x < w - 1 else -1):
            if q < 0 or parent[q] == -2:
                continue
            r = q
            while parent[r] >= 0:
                r = parent[r]
            while parent[q] >= 0:                   # path compression
                parent[q], q = r, parent[q]
            if r == p:
                continue
            if vals[r] == vals[p] or area[r] < lam:
                area[p] += area[r]
                parent[r] = p
            else:
                area[p] = lam                       # p hangs below a component that is large enough already
    out = flat.copy()
    for p in reversed(order):
        if parent[p] >= 0:
            out[p] = out[parent[p]]
    return out.reshape(h, w)


def seed_opening(f, lam):
    f = np.asarray(f)
    assert f.ndim == 2 and f.size >= lam >= 1
    h, w = f.shape
    out = f.copy()
    dirs = ((-1, 0), (1, 0), (0, -1), (0, 1))
    inside = lambda y, x: 0 <= y < h and 0 <= x < w
    for sy in range(h):
        for sx in range(w):
            if any(inside(sy + dy, sx + dx) and f[sy + dy, sx + dx] > f[sy, sx] for dy, dx in dirs):
                continue
            region, cand = [], []                   # growth order; per region pixel the set of directions still frontier
            q = (sy, sx)
            while True:
                for (py, px), c in zip(region, cand):
                    for k, (dy, dx) in enumerate(dirs):
                        if (py + dy, px + dx) == q:
                            c.discard(k)
                fresh = {k for k, (dy, dx) in enumerate(dirs) if inside(q[0] + dy, q[1] + dx) and (q[0] + dy, q[1] + dx) not in region}
                region.append(q)
                cand.append(fresh)
                if len(region) == lam:
                    break
                q = max(((py + dirs[k][0], px + dirs[k][1]) for (py, px), c in zip(region, cand) for k in c), key=lambda t: f[t])
            vals = [f[p] for p in region]
            lvl = min(vals)
            k = next(i for i, v in enumerate(vals) if v <= lvl)
            for p in region[:k]:
                out[p] = lvl
    return out


def closing(f, lam, opening=uf_opening):
    f = np.asarray(f)
    assert f.dtype == np.float32
    one = np.float32(1)
    return one - opening(one - f, lam)
