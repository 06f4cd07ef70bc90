"""Constructed calls of the simulator's sink sampling (csrc/sim_core.h: phase_sample) and a brute-force numpy evaluation of the
reference's expressions (greenhouse.py:319-341, simulation_space.py:89-98) for them. Shared by tests/test_sample_onchip.py (host
builds) and tests/test_sample_onchip_gpu.py (octa_sim_kat_sample); not a test module itself.

A case is a dict: cand [N][3], npos [n][3], nrad [n], oxy [m][3], eps_n, eps_k, eps_s, cst = (param_scale, size x, y, z,
geometry_size, FAZ centre x, y, FAZ radius). With geometry_size = 1 the FAZ test `|xy - centre * gs| > radius * gs / 2` is a disc
of radius / 2 around the centre in the candidates' own units."""
import math

import numpy as np

CH = 2048            # candidates per chunk of the on-chip form (SMP_CH; the host harness reports it, the tests compare)
R0 = 3.5e-3


def oxygen_distance(rad, ps):
    """greenhouse.py:309-317 with the C library's exp, one radius at a time (the host build calls the same function)."""
    kap = 0.02 * 203.9e-3
    out = np.empty(len(rad))
    for i, r in enumerate(rad):
        q = r * ps / R0
        c1 = kap * q * math.exp(1 - q)
        out[i] = c1 * 6 / ps
    return out


def _sqdist(p, q):
    d = p[:, None, :] - q[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def brute_force(case, with_passers=False):
    """The sink list behind the call: the old sinks, then the accepted candidates in candidate order (with_passers: and the number
    of candidates that passed the validity, node and sink tests, i.e. entered the greedy step)."""
    cand, npos, nrad, oxy = case["cand"], case["npos"], case["nrad"], case["oxy"]
    ps, sx, sy, sz, gs, fc0, fc1, faz = case["cst"]
    en, es = max(case["eps_n"], case["eps_k"]), case["eps_s"]
    x, y, z = cand[:, 0], cand[:, 1], cand[:, 2]
    ok = ~((x >= sx) | (y >= sy) | (z >= sz) | (x < 0) | (y < 0) | (z < 0))
    dd = np.sqrt((x - fc0 * gs) * (x - fc0 * gs) + (y - fc1 * gs) * (y - fc1 * gs))
    ok &= dd > faz * gs * 0.5
    oxd = oxygen_distance(nrad, ps)
    for s in range(0, len(cand), 512):
        c = cand[s:s + 512]
        if len(npos):
            d2 = _sqdist(c, npos)
            ok[s:s + 512] &= ~((d2 <= en * en) & ~(np.sqrt(d2) > oxd[None, :])).any(axis=1)
        if len(oxy):
            ok[s:s + 512] &= ~(np.sqrt(_sqdist(c, oxy)) <= es).any(axis=1)
    acc = np.zeros((0, 3))
    for c in cand[ok]:
        d = c[None, :] - acc
        if (np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) > es).all():
            acc = np.vstack([acc, c[None, :]])
    out = np.vstack([oxy.reshape(-1, 3), acc])
    return (out, int(ok.sum())) if with_passers else out


def _pts(rng, n, lo=0.0, hi=1.0):
    p = rng.uniform(lo, hi, (n, 3))
    p[:, 2] = rng.uniform(0, 0.0131, n)
    return np.ascontiguousarray(p)


def random_case(seed, n_cand, n_art, n_oxy, eps_n=0.013, eps_k=0.01, eps_s=0.01, ps=3.0):
    """Uniform candidates a little wider than the domain (some outside on every side), a FAZ disc of radius 0.05, random nodes with
    radii around the oxygen distance's maximum, random sinks."""
    rng = np.random.default_rng(seed)
    cand = _pts(rng, n_cand, -0.02, 1.02)
    cand[:, 2] = rng.uniform(-0.0005, 0.0136, n_cand)
    return dict(cand=cand, npos=_pts(rng, n_art), nrad=rng.uniform(0.0004, 0.004, n_art), oxy=_pts(rng, n_oxy),
                eps_n=eps_n, eps_k=eps_k, eps_s=eps_s, cst=(ps, 1.0, 1.0, 0.0131, 1.0, 0.5, 0.5, 0.1))


def _ulps(v):
    return [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]


def tie_cases():
    """One candidate per call (the greedy step must not hide a flag): at exactly eps_s from a sink, at exactly en from a node whose
    oxygen distance is larger, at exactly the oxygen distance of a node inside en -- each also one ulp nearer and farther. All
    lengths are dyadic or come out of exp(0) = 1 (node radius r0 / ps), so the distances are exact. Yields (name, case)."""
    no_faz = (0.25, 1.0, 1.0, 0.0131, 1.0, 0.5, 0.5, 0.0)
    rad1 = np.array([R0 / 0.25])                         # q = 1: oxygen distance 0.02 * 0.2039 * 6 / 0.25 = 0.097872
    oxd = float(oxygen_distance(rad1, 0.25)[0])
    far = np.array([[0.9, 0.9, 0.005]])
    for k, x in enumerate(_ulps(0.5 + 0.03125)):         # sink at 0.5, eps_s = 2^-5
        yield f"sink_es_{k}", dict(cand=np.array([[x, 0.5, 0.005]]), npos=far, nrad=np.array([1e-4]), oxy=np.array([[0.5, 0.5, 0.005]]),
                                   eps_n=0.0625, eps_k=0.03, eps_s=0.03125, cst=no_faz)
    for k, y in enumerate(_ulps(0.25 + 0.0625)):         # node at 0.25, en = 2^-4 < oxygen distance
        yield f"node_en_{k}", dict(cand=np.array([[0.75, y, 0.005]]), npos=np.array([[0.75, 0.25, 0.005]]), nrad=rad1, oxy=np.zeros((0, 3)),
                                   eps_n=0.0625, eps_k=0.03, eps_s=0.03125, cst=no_faz)
    for k, x in enumerate(_ulps(oxd)):                   # node at x = 0, oxygen distance < en = 2^-3
        yield f"node_oxd_{k}", dict(cand=np.array([[x, 0.5, 0.005]]), npos=np.array([[0.0, 0.5, 0.005]]), nrad=rad1, oxy=np.zeros((0, 3)),
                                    eps_n=0.125, eps_k=0.03, eps_s=0.03125, cst=no_faz)


def border_case():
    """Candidates on the cell borders of the candidate grid (origin -0.1, edge 1.2 / 96 = eps_n), one ulp either side, in the outermost
    cells of the domain and on its faces; nodes and sinks on the same lattice, so that many distances are exactly a radius."""
    e = 1.2 / 96
    ks = np.arange(8, 89)
    g = np.concatenate([(-0.1 + ks * e), np.nextafter(-0.1 + ks * e, 0), np.nextafter(-0.1 + ks * e, 2), [0.0, np.nextafter(1.0, 0), 1.0]])
    rng = np.random.default_rng(77)
    cand = np.stack([rng.choice(g, 1500), rng.choice(g, 1500), rng.uniform(0, 0.0131, 1500)], axis=1)
    cand[:200, 2] = 0.005
    lat = lambda n: np.stack([-0.1 + rng.integers(8, 89, n) * e, -0.1 + rng.integers(8, 89, n) * e, np.full(n, 0.005)], axis=1)
    return dict(cand=np.ascontiguousarray(cand), npos=lat(300), nrad=rng.uniform(0.0004, 0.004, 300), oxy=lat(300),
                eps_n=e, eps_k=0.01, eps_s=e, cst=(3.0, 1.0, 1.0, 0.0131, 1.0, 0.5, 0.5, 0.1))


def mode_switch_case():
    """The first iteration of a mode runs with radii not yet divided by param_scale: a cell edge of 0.18 (7 x 7 cells), about ten
    candidates per cell, every node's and sink's box several cells wide in the other grids' terms."""
    c = random_case(31, 500, 3000, 12, eps_n=0.18, eps_k=0.135, eps_s=0.135)
    return c
