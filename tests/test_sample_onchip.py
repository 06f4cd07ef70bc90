"""CPU: the two forms of the simulator's sink sampling (csrc/sim_core.h: phase_sample) compiled as host C++ with a one-thread block
(tests/native/sample_onchip_host.cpp): the default on-chip form -- candidates binned in the table area, sinks and nodes streamed
past them -- and the direct form behind -DOCTA_SIM_SAMPLE_DIRECT. (a) whole short runs against the golden fixtures, (b) constructed
calls against a brute-force numpy evaluation of the reference's expressions, (c) the conflict rows of the greedy acceptance settled
in rounds against the serial rule."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import yaml

import _sample_cases as SC
from oracle import sim_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "octa_autosegmentation_amd", "csrc")


def _load(so_name, extra):
    src = os.path.join(ROOT, "tests", "native", "sample_onchip_host.cpp")
    so = os.path.join(ROOT, "tests", "native", so_name)
    deps = [src, os.path.join(ROOT, "tests", "native", "sim_core_host.cpp")] + [
        os.path.join(CSRC, f) for f in ("sim_core.h", "sim_host.h", "gpow.h", "glibc_pow_tables.h", "glibc_trig.h", "glibc_trig_tables.h")]
    if not os.path.exists(so) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-fPIC", "-shared"] + extra + ["-o", so, src])
    l = ctypes.CDLL(so)
    l.octa_simcore_host_run.restype = ctypes.c_int
    l.octa_simcore_host_run.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_ulonglong, sim_oracle.BIF_CB, ctypes.c_void_p,
                                        ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p]
    l.octa_sample_host_call.restype = ctypes.c_int
    l.octa_sample_host_call.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                        ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]
    if not extra:
        l.octa_sample_caps.argtypes = [ctypes.c_void_p]
        l.octa_sample_settle.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 4
    return l


@pytest.fixture(scope="module")
def onchip():
    return _load("libsampleonchip.so", [])


@pytest.fixture(scope="module")
def direct():
    return _load("libsampleonchip_direct.so", ["-DOCTA_SIM_SAMPLE_DIRECT"])


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "sim_golden.npz"))


def call(lib, case):
    cand = np.ascontiguousarray(case["cand"], np.float64).reshape(-1, 3)
    npos = np.ascontiguousarray(case["npos"], np.float64).reshape(-1, 3)
    nrad = np.ascontiguousarray(case["nrad"], np.float64)
    oxy0 = np.ascontiguousarray(case["oxy"], np.float64).reshape(-1, 3)
    cap = len(oxy0) + len(cand)
    oxy = np.zeros((cap + 1, 3))
    oxy[: len(oxy0)] = oxy0
    cst = np.array(case["cst"], np.float64)
    n = lib.octa_sample_host_call(cand.ctypes.data, len(cand), npos.ctypes.data, nrad.ctypes.data, len(npos), oxy.ctypes.data, len(oxy0), cap,
                                  case["eps_n"], case["eps_k"], case["eps_s"], cst.ctypes.data)
    assert n >= len(oxy0), n
    return oxy[:n]


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_capacity_is_what_the_cases_assume(onchip):
    caps = np.zeros(3, np.int32)
    onchip.octa_sample_caps(caps.ctypes.data)
    assert caps[0] == SC.CH and caps[1] == 1024 and caps[2] == 2048


def test_short_runs_equal_the_golden_in_both_forms(onchip, direct, golden):
    """run_s0_30_20 crosses the mode switch (30 + 20 iterations), run_s5_10_5 is the short one: traces, every double of the edge lists
    and the CSV bytes."""
    for name in ("run_s0_30_20", "run_s5_10_5"):
        seed, i1, i2 = (int(v) for v in golden[name + "_seed_I"])
        cfg = yaml.safe_load(str(golden["config_yaml"]))
        cfg["Greenhouse"]["modes"][0]["I"] = i1
        cfg["Greenhouse"]["modes"][1]["I"] = i2
        p = sim_oracle.params_from_config(cfg)
        got = []
        for lib in (onchip, direct):
            edges = np.zeros((40000, 7)); trace = np.zeros((i1 + i2, 4), np.int64); info = np.zeros(8, np.int64)
            rc = lib.octa_simcore_host_run(ctypes.addressof(p), seed, seed, sim_oracle._bif_cb, edges.ctypes.data, 40000, trace.ctypes.data, info.ctypes.data)
            assert rc == 0 and info[2] == 0
            assert (trace[: info[7]] == golden[name + "_trace"]).all(), name
            assert sim_oracle.edges_to_csv_text(edges[: info[0]]).encode() == golden[name + "_csv"].tobytes(), name
            got.append((trace.copy(), edges[: info[0]].copy()))
        assert same(got[0][0], got[1][0]) and same(got[0][1], got[1][1]), name


@pytest.fixture(scope="module")
def chunk_cases():
    """N = 0, 1, the chunk capacity, capacity + 1 and three times the capacity, against 3000 nodes and 5000 sinks; the brute force once."""
    out = []
    for k, n in enumerate((0, 1, SC.CH, SC.CH + 1, 3 * SC.CH)):
        c = SC.random_case(100 + k, n, 3000, 5000)
        out.append((n, c, SC.brute_force(c)))
    return out


def test_chunks_against_brute_force(onchip, direct, chunk_cases):
    for n, c, want in chunk_cases:
        assert n < 2 or len(want) > 5000 + n // 40, "the case accepts too few candidates to say anything"
        assert same(call(onchip, c), want), n
        assert same(call(direct, c), want), n


def test_no_sinks_and_sixteen_nodes(onchip, direct):
    """n_oxy = 0 and the 16 stump nodes of a fresh sample; with eps_s small nearly every candidate passes: more passers than the greedy
    step's table holds (one chunk: the passers go to scratch by a second compaction; three chunks: they are there already), so the
    one-candidate-after-the-other loop decides."""
    for n in (300, SC.CH, 3 * SC.CH):
        c = SC.random_case(7 + n, n, 16, 0, eps_s=0.004 if n <= SC.CH else 0.016)      # (at most 2048 are accepted per call)
        want, n_pass = SC.brute_force(c, with_passers=True)
        assert (n < SC.CH or n_pass > 1024) and len(want) <= 2048
        assert same(call(onchip, c), want), n
        assert same(call(direct, c), want), n


def test_pair_list_overflow_falls_back(onchip, direct):
    """1000 passers of which most pairs conflict (eps_s = 0.2): the pair list (2048) overflows and the serial loop takes over."""
    c = SC.random_case(9, 1000, 16, 0, eps_n=0.004, eps_k=0.2, eps_s=0.2)
    c["nrad"][:] = 1e-5                      # oxygen distance ~ 2e-4: the nodes reject next to nothing
    want, n_pass = SC.brute_force(c, with_passers=True)
    assert 5 < len(want) < 60 and 800 < n_pass <= 1024
    assert same(call(onchip, c), want) and same(call(direct, c), want)


def test_ties_at_the_radii(onchip, direct):
    got = {}
    for name, c in SC.tie_cases():
        want = SC.brute_force(c)
        assert same(call(onchip, c), want) and same(call(direct, c), want), name
        got[name] = len(want) - len(c["oxy"])
    # at the radius itself and one ulp inside the candidate is rejected, one ulp outside it is accepted
    for kind in ("sink_es", "node_en", "node_oxd"):
        assert [got[f"{kind}_{k}"] for k in range(3)] == [0, 0, 1], (kind, got)


def test_cell_borders_faz_and_mode_switch(onchip, direct):
    for name, c in (("border", SC.border_case()), ("mode switch", SC.mode_switch_case())):
        want = SC.brute_force(c)
        assert len(want) > len(c["oxy"]) + 3, name
        assert same(call(onchip, c), want) and same(call(direct, c), want), name
    # candidates inside the FAZ disc (radius 0.05 around the centre) and outside the domain are never accepted
    c = SC.random_case(5, 600, 16, 0, eps_s=0.002)
    c["cand"][:200, :2] = 0.5 + np.random.default_rng(1).uniform(-0.07, 0.07, (200, 2))
    want = SC.brute_force(c)
    acc = want[len(c["oxy"]):]
    assert len(acc) > 300 and (np.hypot(acc[:, 0] - 0.5, acc[:, 1] - 0.5) > 0.05).all() and (acc >= 0).all() and (acc[:, :2] < 1).all()
    assert same(call(onchip, c), want) and same(call(direct, c), want)


def _serial_settle(lists):
    st = []
    for l in lists:
        st.append(2 if any(st[i] == 1 for i in l) else 1)
    return st


def _settle(lib, lists):
    n = len(lists)
    rcnt = np.array([len(l) for l in lists], np.uint16)
    order = np.random.default_rng(n).permutation(n)            # the device lists the rows in the order their threads arrive
    rstart = np.zeros(n, np.uint16); pl = np.zeros(max(1, int(rcnt.sum())), np.uint16)
    at = 0
    for j in order:
        rstart[j] = at
        pl[at: at + len(lists[j])] = lists[j]
        at += len(lists[j])
    state = np.full(n, 9, np.uint8)
    assert lib.octa_sample_settle(n, rcnt.ctypes.data, rstart.ctypes.data, pl.ctypes.data, state.ctypes.data) == 0
    return state.tolist()


def test_conflict_rows_settle_as_the_serial_rule(onchip):
    # chains of depth 1 .. 6: row j lists row j - 1
    for depth in range(1, 7):
        lists = [[]] + [[j - 1] for j in range(1, depth + 1)]
        assert _settle(onchip, lists) == _serial_settle(lists) == [1 if j % 2 == 0 else 2 for j in range(depth + 1)]
    # a row whose listed rows are all rejected is accepted
    lists = [[], [0], [0], [1, 2], [3], []]
    assert _settle(onchip, lists) == [1, 2, 2, 1, 2, 1]
    rng = np.random.default_rng(3)
    for n, p in ((1, 0.0), (64, 0.05), (65, 0.3), (300, 0.01), (1024, 0.003), (200, 0.08)):
        lists = [sorted(int(i) for i in np.nonzero(rng.uniform(size=j) < p)[0]) for j in range(n)]
        assert sum(len(l) for l in lists) <= 2048
        assert _settle(onchip, lists) == _serial_settle(lists), (n, p)
