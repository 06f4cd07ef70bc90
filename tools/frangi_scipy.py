"""tools/frangi_scipy.py -- scikit-image >= 0.25's 2-D `skimage.filters.frangi`, restated over scipy.ndimage and numpy for the
build container (scikit-image is absent there). tools/make_golden_frangi.py registers `frangi` below as `skimage.filters.frangi`,
so the reference's models/frangi.py runs unchanged on it. Parity with scikit-image itself is NOT pinned by this file.

What it follows, statement by statement:
  frangi()                   image.astype(float32); -image when black_ridges is False; per sigma: eigenvalues of the Hessian sorted
                             by magnitude (abs().argsort(0), stable for two values), lambda2 = maximum(lambda2, 1e-10),
                             r_b = |lambda1| / lambda2, s = sqrt(sum(eigvals ** 2)), gamma = s.max() / 2 (1 when that is 0) fixed at
                             the FIRST sigma, vals = (1.0 - exp(-inf)) * exp(-r_b^2 / (2 beta^2)) * (1.0 - exp(-s^2 / (2 gamma^2)))
                             -- the first factor is a float64 scalar, so the products are float64 -- and the maximum over sigmas.
  hessian_matrix(..., use_gaussian_derivatives=True)
                             five ndimage.gaussian_filter calls at sigma / sqrt(2), truncate 8 (sigma > 1) or 100: the two
                             gradients, then a first-order derivative of each gradient (rr, rc, cc), all float32.
  hessian_matrix_eigvals()   (M00 + M11) / 2 +- sqrt(M01 ** 2 + ((M00 - M11) / 2) ** 2), float32.
`trace`, when a list, receives per sigma a dict of the Hessian planes, the sorted eigenvalues and gamma."""
import math
from itertools import combinations_with_replacement

import numpy as np
from scipy import ndimage as ndi


def hessian_matrix(image, sigma, mode="reflect", cval=0):
    image = image.astype(np.float32, copy=False)
    sigma_scaled = ((1 / math.sqrt(2)) * sigma,) * image.ndim
    truncate = 8 if sigma > 1 else 100

    def gaussian(x, order):
        return ndi.gaussian_filter(x, sigma=sigma_scaled, order=order, mode=mode, cval=cval, truncate=truncate)

    ndim = image.ndim
    orders = tuple([0] * d + [1] + [0] * (ndim - d - 1) for d in range(ndim))
    gradients = [gaussian(image, orders[d]) for d in range(ndim)]
    return [gaussian(gradients[a0], orders[a1]) for a0, a1 in combinations_with_replacement(range(ndim), 2)]


def hessian_matrix_eigvals(H):
    M00, M01, M11 = H
    eigs = np.empty((2, *M00.shape), M00.dtype)
    eigs[:] = (M00 + M11) / 2
    hsqrtdet = np.sqrt(M01 ** 2 + ((M00 - M11) / 2) ** 2)
    eigs[0] += hsqrtdet
    eigs[1] -= hsqrtdet
    return eigs


def frangi(image, sigmas=range(1, 10, 2), scale_range=None, scale_step=None, alpha=0.5, beta=0.5, gamma=None, black_ridges=True,
           mode="reflect", cval=0, trace=None):
    if image.ndim != 2:
        raise ValueError("this restatement covers 2-D images only")
    image = image.astype(np.float32, copy=False)
    if not black_ridges:
        image = -image
    filtered_max = np.zeros_like(image)
    for sigma in sigmas:
        H = hessian_matrix(image, sigma, mode=mode, cval=cval)
        eigvals = hessian_matrix_eigvals(H)
        eigvals = np.take_along_axis(eigvals, abs(eigvals).argsort(0), 0)
        lambda1 = eigvals[0]
        (lambda2,) = np.maximum(eigvals[1:], 1e-10)
        r_a = np.inf
        r_b = abs(lambda1) / lambda2
        s = np.sqrt((eigvals ** 2).sum(0))
        if gamma is None:
            gamma = s.max() / 2
            if gamma == 0:
                gamma = 1
        vals = 1.0 - np.exp(-(r_a ** 2) / (2 * alpha ** 2))
        vals *= np.exp(-(r_b ** 2) / (2 * beta ** 2))
        vals *= 1.0 - np.exp(-(s ** 2) / (2 * gamma ** 2))
        if trace is not None:
            trace.append({"sigma": sigma, "hrr": H[0], "hrc": H[1], "hcc": H[2], "l1": eigvals[0].copy(), "l2": eigvals[1].copy(),
                          "gamma": gamma, "vals": vals})
        filtered_max = np.maximum(filtered_max, vals)
    return filtered_max
