"""CPU: the three-rung ladder of the O2 -> CO2 conversion (phase_satisfy_art, csrc/sim_core.h) on the host build of the phase code
(tests/native/kd_partial_host.cpp): set order certified without the kd order / kd ranks for the flagged groups only / full kd order.
The plain build, -DOCTA_SIM_KD_NOPARTIAL (the two-rung form), -DOCTA_SIM_KD_PARTIAL_REFUSE (the second certificate always refuses,
so the full build runs behind every partial one) and -DOCTA_SIM_KD_SPARSE=0 (kd_build never walks a level's listed ranges only) must all print the reference's bytes and equal the oracle in every double; and
kd_build with a sparse `need` mask must put the needed points where scipy's cKDTree does."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import yaml

from oracle import sim_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": [], "nopartial": ["-DOCTA_SIM_KD_NOPARTIAL"], "refuse": ["-DOCTA_SIM_KD_PARTIAL_REFUSE"],
          "nosparse": ["-DOCTA_SIM_KD_SPARSE=0"]}      # kd_build's box and key passes always walk [0, n)
# name -> (seed, I of mode 0, I of mode 1, golden fixture with the reference's bytes or None)
CASES = {"run_s0_30_20": (0, 30, 20, True), "run_s3_30_20": (3, 30, 20, True),
         "s0_100_20": (0, 100, 20, False),           # across the mode switch: iteration 100 has thousands of hits
         "s1000_full": (1000, 100, 150, False)}      # one full-length sample


def load(so_name, extra_flags):
    src = os.path.join(ROOT, "tests", "native", "kd_partial_host.cpp")
    so = os.path.join(ROOT, "tests", "native", so_name)
    deps = [src] + [os.path.join(ROOT, "octa_autosegmentation_amd", "csrc", f) for f in ("sim_core.h", "sim_host.h", "gpow.h", "glibc_pow_tables.h", "glibc_trig.h", "glibc_trig_tables.h")]
    if not os.path.exists(so) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-fPIC", "-shared"] + extra_flags + ["-o", so, src])
    l = ctypes.CDLL(so)
    l.octa_kdpartial_host_run.restype = ctypes.c_int
    l.octa_kdpartial_host_run.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_ulonglong, sim_oracle.BIF_CB, ctypes.c_void_p,
                                          ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p]
    l.octa_kdpartial_kd_indices.restype = None
    l.octa_kdpartial_kd_indices.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return l


def config(golden, i1, i2):
    cfg = yaml.safe_load(str(golden["config_yaml"]))
    cfg["Greenhouse"]["modes"][0]["I"] = int(i1)
    cfg["Greenhouse"]["modes"][1]["I"] = int(i2)
    return cfg


def host_run(lib, golden, name):
    """-> (edges, trace, (certified, partial, full))"""
    seed, i1, i2, _ = CASES[name]
    p = sim_oracle.params_from_config(config(golden, i1, i2))
    edges = np.zeros((40000, 7))
    trace = np.zeros((i1 + i2, 4), np.int64)
    info = np.zeros(11, np.int64)
    rc = lib.octa_kdpartial_host_run(ctypes.addressof(p), seed, seed, sim_oracle._bif_cb, edges.ctypes.data, 40000, trace.ctypes.data, info.ctypes.data)
    assert rc == 0 and info[2] == 0, (name, rc, info)
    return edges[: info[0]].copy(), trace[: info[7]].copy(), tuple(int(v) for v in info[8:11])


@pytest.fixture(scope="module")
def libs():
    return {k: load(f"libkdpartialhost_{k}.so", flags) for k, flags in BUILDS.items()}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "sim_golden.npz"))


@pytest.fixture(scope="module")
def oracle_runs(golden):
    out = {}
    for name, (seed, i1, i2, _) in CASES.items():
        edges, info = sim_oracle.simulate(config(golden, i1, i2), seed)
        out[name] = (edges, info["trace"])
    return out


@pytest.fixture(scope="module")
def runs(libs, golden):
    return {(k, name): host_run(lib, golden, name) for k, lib in libs.items() for name in CASES}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("build", list(BUILDS))
def test_every_build_gives_the_reference_bytes_and_the_oracles_doubles(runs, oracle_runs, golden, build, name):
    edges, trace, _ = runs[(build, name)]
    e_or, t_or = oracle_runs[name]
    assert (trace == t_or).all()
    assert e_or.shape == edges.shape and e_or.tobytes() == edges.tobytes()
    if CASES[name][3]:
        assert (trace == golden[name + "_trace"]).all()
        assert sim_oracle.edges_to_csv_text(edges).encode() == golden[name + "_csv"].tobytes()


@pytest.mark.parametrize("name", list(CASES))
def test_the_partial_rung_is_taken_and_the_builds_count_alike(runs, name):
    cert, part, full = runs[("plain", name)][2]
    print(f"{name}: plain build certified {cert} / partial {part} / full {full};"
          f" refuse build {runs[('refuse', name)][2]}; two-rung build {runs[('nopartial', name)][2]}")
    assert part > 0
    # the second certificate refuses always: every partial build is followed by the full one
    assert runs[("refuse", name)][2] == (cert, 0, part + full)
    # the two-rung form refuses the same conversions
    assert runs[("nopartial", name)][2] == (cert, 0, part + full)
    assert runs[("nosparse", name)][2] == (cert, part, full)


# ---- kd_build with a sparse `need`
def _points(rng, n, clustered):
    if clustered:
        k = 1 + n // 500
        centres = rng.uniform(0.1, 0.9, (k, 3))
        pts = centres[rng.integers(0, k, n)] + rng.uniform(-1, 1, (n, 3)) * 10.0 ** rng.uniform(-10, -2, (n, 1))
    else:
        pts = rng.uniform(0, 1, (n, 3))
    return np.ascontiguousarray(np.abs(pts) * np.array([1, 1, 0.0131]))


def need_cases():
    """(n, clustered, needed point ids): 1, 2 and 9 needed points, the 9 partly next to one another in space"""
    rng = np.random.default_rng(77)
    for n in (17, 40, 300, 4001, 13312):
        for clustered in (False, True):
            pts = _points(rng, n, clustered)
            for k in (1, 2, 9):
                ids = rng.choice(n, min(k, n), replace=False)
                if k == 9:      # five of them: the nearest neighbours of the first
                    near = np.argsort(((pts - pts[ids[0]]) ** 2).sum(axis=1))[1:6]
                    ids = np.unique(np.concatenate([ids[:4], near]))
                yield pts, ids


@pytest.mark.parametrize("build", ["plain", "nosparse"])
def test_sparse_need_puts_the_needed_points_at_scipys_positions(libs, build):
    """With the walk over the listed ranges of a sparse level (plain) and with the walk over [0, n) at every level (nosparse)."""
    from scipy.spatial import cKDTree
    lib = libs[build]
    for pts, ids in need_cases():
        n = len(pts)
        want = cKDTree(pts).indices
        need = np.zeros(n, np.uint8)
        need[::3] = 1               # bit 0 set on other points: not selected by need_bits = 2
        need[ids] |= 2
        idx, rank = np.zeros(n, np.uint16), np.zeros(n, np.uint16)
        lib.octa_kdpartial_kd_indices(pts.ctypes.data, n, need.ctypes.data, 2, idx.ctypes.data, rank.ctypes.data)
        assert sorted(idx.tolist()) == list(range(n))                  # a permutation, and rank its inverse
        assert (idx[rank] == np.arange(n)).all()
        pos = np.empty(n, np.int64)
        pos[want] = np.arange(n)
        assert (rank[ids] == pos[ids]).all(), (n, ids.tolist())
        # every bit counts: the points flagged with bit 0 stand at their positions too
        lib.octa_kdpartial_kd_indices(pts.ctypes.data, n, need.ctypes.data, 0xff, idx.ctypes.data, rank.ctypes.data)
        sel = np.flatnonzero(need)
        assert (rank[sel] == pos[sel]).all(), n
