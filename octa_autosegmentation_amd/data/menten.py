"""Host side of the Menten et al. (MICCAI 2022) augmentation -- the reference's comparison baseline `MentenAugmentationd`
(reference data/data_transforms.py:44-325: BinomialVesselNoised, AddVitreousFloater, AddMotionArtifact).

Three things live here, shared by the transforms of data/data_transforms.py, the fixture generator and the tests:
* the DRAWS: every random number comes from numpy's global legacy stream through the reference's own calls in the reference's own
  order, so the stream ends where the reference's ends, whichever path then does the arithmetic;
* the HOST RESTATEMENT of the arithmetic (numpy + scipy.ndimage, the reference's own expressions: bit-identical by construction),
  taken by CPU tensors and by layouts outside the kernels of csrc/menten.hip;
* what the kernels need from the host: scipy's Gaussian taps, the cuts of a motion call folded into a per-row gather table.

`draw_line` restates skimage.draw.line (Bresenham, both end points included). skimage is neither installed here nor shipped with the
reference: parity with skimage ITSELF is UNPINNED (as for MONAI, data/data_transforms.py); the restatement follows skimage's published
algorithm (skimage/draw/_draw.pyx `_line`) and is pinned against hand-written point lists (tests/test_menten.py). The fixtures of
tests/golden/menten_golden.npz were produced by the reference's classes with this function injected as `skimage.draw.line`.
"""
import numpy as np


def _ndimage():
    try:
        import scipy.ndimage as ndi
    except ImportError as e:            # pragma: no cover -- scipy is a dependency of the host path only
        raise ImportError("the host path of the Menten augmentation (CPU tensors, layouts outside csrc/menten.hip) needs scipy.ndimage "
                          "(binary_dilation, gaussian_filter); install scipy or hand the transforms CUDA tensors [1, H, W]") from e
    return ndi


def draw_line(r0, c0, r1, c1):
    """skimage.draw.line: (rr, cc) of the Bresenham line from (r0, c0) to (r1, c1), max(|dr|, |dc|) + 1 points, both ends included."""
    r0, c0, r1, c1 = int(r0), int(c0), int(r1), int(c1)
    steep = False
    r, c = r0, c0
    dr, dc = abs(r1 - r0), abs(c1 - c0)
    sc = 1 if (c1 - c) > 0 else -1
    sr = 1 if (r1 - r) > 0 else -1
    if dr > dc:
        steep = True
        c, r = r, c
        dc, dr = dr, dc
        sc, sr = sr, sc
    d = 2 * dr - dc
    rr = np.zeros(dc + 1, dtype=np.intp)
    cc = np.zeros(dc + 1, dtype=np.intp)
    for i in range(dc):
        if steep:
            rr[i], cc[i] = c, r
        else:
            rr[i], cc[i] = r, c
        while d >= 0:
            r += sr
            d -= 2 * dc
        c += sc
        d += 2 * dr
    rr[dc], cc[dc] = r1, c1
    return rr, cc


def gaussian_radius(sigma, truncate=4.0):
    return int(truncate * float(sigma) + 0.5)


def gaussian_weights(sigma, truncate=4.0):
    """The taps scipy.ndimage.gaussian_filter1d correlates with (order 0): exp(-x^2 / (2 sigma^2)) over [-radius, radius], divided by
    their sum -- computed with scipy's own expressions (scipy/ndimage/_filters.py `_gaussian_kernel1d`)."""
    sigma = float(sigma)
    radius = gaussian_radius(sigma, truncate)
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    return phi_x / phi_x.sum()


# ---- BinomialVesselNoised ------------------------------------------------------------------------------------------------------------

def vessel_noise_host(img, vessel_noise_scaling=0.5, vessel_noise_blur=1.0, r=48):
    """reference :54-92 `add_noise` on a 2-D numpy image; the per-pixel Python loop over the five rings is stated on whole arrays with the
    same float64 operations (sqrt of the same sum, strict compare, one multiplication by 0.7 per ring)."""
    ndi = _ndimage()
    vessel_noise = np.random.binomial(1, 0.1, size=img.shape)
    vessel_noise = ndi.binary_dilation(vessel_noise, iterations=1).astype(float)
    i = np.arange(vessel_noise.shape[0], dtype=np.float64)[:, None]
    j = np.arange(vessel_noise.shape[1], dtype=np.float64)[None, :]
    dist = np.sqrt((i - vessel_noise.shape[0] / 2) ** 2 + (j - vessel_noise.shape[1] / 2) ** 2)
    for m in range(5):
        vessel_noise = np.where(dist < r - 3 * m, vessel_noise * 0.7, vessel_noise)
    vessel_noise = ndi.gaussian_filter(vessel_noise, vessel_noise_blur) * vessel_noise_scaling
    quantum_noise = np.random.uniform(0.0, 0.2, size=img.shape)
    return np.clip((img + vessel_noise + quantum_noise) / (1.0 + vessel_noise_scaling / 1.5), 0.0, 1.0)


def vessel_noise_draws(shape):
    """The two fields of `add_noise`, in its order: binomial(1, 0.1) as uint8, uniform(0, 0.2) as float64."""
    bern = np.random.binomial(1, 0.1, size=shape)
    quantum = np.random.uniform(0.0, 0.2, size=shape)
    return bern.astype(np.uint8), quantum


# ---- AddVitreousFloater --------------------------------------------------------------------------------------------------------------

def floater_draws(H, W, floater_chance=0.1, floater_opacity_interval=(0.5, 1.0), floater_segments_interval=(10, 20), dilations_interval=(10, 30)):
    """reference :147-180. None when no floater is added (one uniform() drawn); else (points int32 [n + 1, 2], opacity, dilations). A point is
    (index along the mask's first axis, index along its second): the reference allocates the mask as (W, H) and walks it with
    (x in [0, W), y in [0, H))."""
    if not (np.random.uniform() < floater_chance):
        return None
    size_x, size_y = W, H
    starting_x = np.random.randint(0, size_x)
    starting_y = np.random.randint(0, size_y)
    current = np.array((starting_x, starting_y))
    points = [current]
    opacity = np.random.uniform(*floater_opacity_interval)          # drawn, but without effect: the dilation makes the mask boolean
    segments = np.random.randint(*floater_segments_interval)
    for _ in range(segments):
        dx = int(np.random.normal(scale=size_x / 10))
        dy = int(np.random.normal(scale=size_y / 10))
        current = current + (dx, dy)
        points.append(current)
    dilations = np.random.randint(*dilations_interval)
    return np.asarray(points, dtype=np.int32).reshape(-1, 2), opacity, int(dilations)


def floater_lines_host(points, opacity, H, W):
    """The (W, H) float mask with `opacity` on every segment's Bresenham pixels inside the image (reference :151-178)."""
    size_x, size_y = W, H
    floater = np.zeros((size_x, size_y))
    for a, b in zip(points[:-1], points[1:]):
        rr, cc = draw_line(a[0], a[1], b[0], b[1])
        inside = np.logical_and.reduce((rr >= 0, rr < size_x, cc >= 0, cc < size_y))
        floater[rr[inside], cc[inside]] = opacity
    return floater


def floater_host(img, draws):
    """reference :181-184 on a 2-D numpy image with the draws of floater_draws. H != W raises numpy's broadcasting ValueError, as there."""
    ndi = _ndimage()
    points, opacity, dilations = draws
    floater = floater_lines_host(points, opacity, img.shape[0], img.shape[1])
    floater = ndi.binary_dilation(floater, iterations=dilations).astype(float)
    floater = ndi.gaussian_filter(floater, 10)
    return img * (1 - floater)


# ---- AddMotionArtifact ---------------------------------------------------------------------------------------------------------------

def motion_draws(H, W, artifacts, grace_margin=10, max_shear=5, max_stretch=5, max_buckle=5, max_whiteout=1, no_h_cuts=3):
    """reference :262-301: [(kind, position, amount, whiteout rows float64 [amount, W] or None)] in the order of the cuts."""
    cuts = []
    for _ in range(np.random.randint(0, no_h_cuts)):
        artifact = str(np.random.choice(list(artifacts.keys()), p=list(artifacts.values())))
        position = int(np.random.randint(grace_margin, H - grace_margin))
        amount, rows = 0, None
        if artifact == 'shear':
            amount = int(np.random.randint(0, max_shear + 1))
        elif artifact == 'stretch':
            amount = int(np.random.randint(1, max_stretch + 1))
        elif artifact == 'buckle':
            amount = int(np.random.randint(1, max_buckle + 1))
        elif artifact == 'whiteout':
            amount = int(np.random.randint(1, max_whiteout + 1))
            rows = np.random.uniform(0.5, 1.0, size=(amount, W))
        cuts.append((artifact, position, amount, rows))
    return cuts


def motion_host(img, gt, cuts):
    """reference :266-301 with the draws of motion_draws, each cut applied to the result of the previous one. img [H, W] and gt [4H, 4W] (or
    whatever the caller has: the slices are the reference's) are numpy arrays the caller owns; they are changed in place and returned."""
    for artifact, position, amount, rows in cuts:
        temp_img = img.copy()
        temp_gt = gt.copy()
        if artifact == 'shear':
            shear = amount
            img[:position, :] = temp_img[:position, :]
            img[position:, :] = np.roll(temp_img[position:, :], shear, axis=1)
            img[position:, :shear] = 0
            gt[:4 * position, :] = temp_gt[:4 * position, :]
            gt[4 * position:, :] = np.roll(temp_gt[4 * position:, :], 4 * shear, axis=1)
            gt[4 * position:, :4 * shear] = 0
        elif artifact == 'stretch':
            stretch = amount
            img[:position, :] = temp_img[:position, :]
            img[position:position + stretch, :] = temp_img[position, :]
            img[position + stretch:, :] = temp_img[position:-stretch, :]
            gt[:4 * position, :] = temp_gt[:4 * position, :]
            gt[4 * position:4 * position + 4 * stretch, :] = temp_gt[4 * position, :]
            gt[4 * position + 4 * stretch:, :] = temp_gt[4 * position:-4 * stretch, :]
        elif artifact == 'buckle':
            buckle = amount
            img[:position, :] = temp_img[:position, :]
            img[position:, :] = temp_img[position - buckle:-buckle, :]
            gt[:4 * position, :] = temp_gt[:4 * position, :]
            gt[4 * position:, :] = temp_gt[4 * position - 4 * buckle:-4 * buckle, :]
        elif artifact == 'whiteout':
            img[position:position + amount, :] = rows
    return img, gt


def fold_cuts(H, W, cuts, scale=1):
    """The cuts of one call as ONE gather: table int32 [H * scale, 2] = (source, shift) per output row, out[R][j] = 0 for j < shift, else
    source[j - shift], where source >= 0 is that row of the input and source < 0 is whiteout row -source - 1 of the returned list
    (float64 [k, W]; a whiteout touches the image only, so scale must be 1 for it to count). The reference's slice assignments are
    applied to the row descriptors instead of the pixels: np.roll by s followed by zeroing the first s columns is "shift by s with a
    zero prefix" (the wrapped columns are exactly the zeroed ones), and shifts of successive shears add up. Positions and amounts are
    multiplied by `scale` (4 for the label)."""
    n = H * scale
    src, shift = np.arange(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    white = []
    for artifact, position, amount, rows in cuts:
        p, a = position * scale, amount * scale
        ts, th = src.copy(), shift.copy()
        if artifact == 'shear':
            shift[p:] = th[p:] + a
        elif artifact == 'stretch':
            for arr, t in ((src, ts), (shift, th)):
                arr[p:p + a] = t[p]
                arr[p + a:] = t[p:-a]
        elif artifact == 'buckle':
            for arr, t in ((src, ts), (shift, th)):
                arr[p:] = t[p - a:-a]
        elif artifact == 'whiteout' and scale == 1:
            src[p:p + a] = -(len(white) + np.arange(a)) - 1
            shift[p:p + a] = 0
            white.extend(rows)
    table = np.stack([src, np.minimum(shift, W * scale)], axis=1).astype(np.int32)
    return table, (np.stack(white) if white else None)
