"""GPU: one call of the simulator's sink sampling (csrc/sim_core.h: phase_sample, the on-chip form of the default build) in one
workgroup through octa_sim_kat_sample, against the brute-force numpy evaluation of the reference's expressions in
tests/_sample_cases.py: the accepted list in order and in every double. Every input runs twice: the sinks and nodes clear the
candidates' live bytes concurrently by design, and the result must not depend on who comes first."""
import numpy as np
import pytest

import _sample_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kat(hip_lib_built):
    import torch
    assert torch.cuda.is_available()
    from octa_autosegmentation_amd import _native
    L, ctx = _native.lib(), _native.ctx()

    def run(case):
        cand = np.ascontiguousarray(case["cand"], np.float64).reshape(-1, 3)
        npos = np.ascontiguousarray(case["npos"], np.float64).reshape(-1, 3)
        nrad = np.ascontiguousarray(case["nrad"], np.float64)
        oxy0 = np.ascontiguousarray(case["oxy"], np.float64).reshape(-1, 3)
        cap = len(oxy0) + len(cand)
        oxy = np.zeros((cap + 1, 3))
        oxy[: len(oxy0)] = oxy0
        cst = np.array(case["cst"], np.float64)
        n = np.zeros(1, np.int64)
        _native.check(L.octa_sim_kat_sample(ctx, cand.ctypes.data, len(cand), npos.ctypes.data, nrad.ctypes.data, len(npos), oxy.ctypes.data, len(oxy0), cap,
                                            case["eps_n"], case["eps_k"], case["eps_s"], cst.ctypes.data, n.ctypes.data), "octa_sim_kat_sample")
        assert len(oxy0) <= n[0] <= cap
        return oxy[: n[0]].copy()
    return run


def check(kat, case, want, tag):
    a, b = kat(case), kat(case)
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), (tag, "two runs differ")
    assert a.shape == want.shape and a.tobytes() == want.tobytes(), tag


@pytest.mark.parametrize("n_oxy", (0, 5000))
@pytest.mark.parametrize("n_art", (16, 3000))
def test_shapes_against_brute_force(kat, n_art, n_oxy):
    """N = 1, 300, the chunk capacity and capacity + 1 (two chunks). Without sinks nearly every candidate passes: more passers than
    the greedy step's table holds, the one-wave loop decides."""
    for n in (1, 300, SC.CH, SC.CH + 1):
        c = SC.random_case(1000 + n + n_art + n_oxy, n, n_art, n_oxy)
        want, n_pass = SC.brute_force(c, with_passers=True)
        assert n < SC.CH or (n_pass > 1024) == (n_oxy == 0)
        check(kat, c, want, (n, n_art, n_oxy))


def test_three_chunks_and_the_fallbacks(kat):
    c = SC.random_case(104, 3 * SC.CH, 3000, 5000)
    check(kat, c, SC.brute_force(c), "three chunks")
    c = SC.random_case(7 + 3 * SC.CH, 3 * SC.CH, 16, 0, eps_s=0.016)
    check(kat, c, SC.brute_force(c), "three chunks, passers beyond the table")
    c = SC.random_case(9, 1000, 16, 0, eps_n=0.004, eps_k=0.2, eps_s=0.2)
    c["nrad"][:] = 1e-5
    check(kat, c, SC.brute_force(c), "pair list overflow")


def test_ties_borders_and_the_mode_switch(kat):
    got = {}
    for name, c in SC.tie_cases():
        want = SC.brute_force(c)
        check(kat, c, want, name)
        got[name] = len(want) - len(c["oxy"])
    for kind in ("sink_es", "node_en", "node_oxd"):
        assert [got[f"{kind}_{k}"] for k in range(3)] == [0, 0, 1], (kind, got)
    for name, c in (("border", SC.border_case()), ("mode switch", SC.mode_switch_case())):
        check(kat, c, SC.brute_force(c), name)
