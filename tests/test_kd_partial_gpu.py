"""GPU: the three-rung ladder of the O2 -> CO2 conversion (phase_satisfy_art, csrc/sim_core.h) in the device build: the reference's bytes
on the short fixtures and across the mode switch, the same three path counts (certified / partial kd order / full kd order) as the host
build of tests/test_kd_partial.py for the same seed, run-to-run equality with two samples per CU, and kd_build with a sparse `need`
mask against scipy."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = ("run_s0_30_20", "run_s3_30_20", "s0_100_20")


@pytest.fixture(scope="module")
def host():
    import test_kd_partial
    return test_kd_partial


@pytest.fixture(scope="module")
def golden(host):
    import os
    return np.load(os.path.join(host.ROOT, "tests", "golden", "sim_golden.npz"))


@pytest.fixture(scope="module")
def gh(hip_lib_built):
    import torch
    assert torch.cuda.is_available()
    from octa_autosegmentation_amd.vessel_graph_generation import greenhouse
    return greenhouse


def _kd_paths(sim, n):
    from octa_autosegmentation_amd import _native
    paths = np.zeros((n, 3), np.int64)
    _native.check(sim._lib.octa_sim_kd_paths(sim._h, paths.ctypes.data), "octa_sim_kd_paths")
    return paths


def test_sparse_need_puts_the_needed_points_at_scipys_positions(hip_lib_built, host):
    from scipy.spatial import cKDTree
    from octa_autosegmentation_amd import _native
    L, ctx = _native.lib(), _native.ctx()
    for pts, ids in host.need_cases():
        n = len(pts)
        need = np.zeros(n, np.uint8)
        need[ids] = 1
        out = np.zeros(n, np.int32)
        _native.check(L.octa_sim_kat_kd_order(ctx, pts.ctypes.data, n, need.ctypes.data, out.ctypes.data), "octa_sim_kat_kd_order")
        assert sorted(out.tolist()) == list(range(n))
        want = cKDTree(pts).indices
        pos, got = np.empty(n, np.int64), np.empty(n, np.int64)
        pos[want] = np.arange(n)
        got[out] = np.arange(n)
        assert (got[ids] == pos[ids]).all(), (n, ids.tolist())
        # the form phase_satisfy_art calls: the flag in the sign of x, bit 1 of the need byte; bit 0 set on other points does not count
        need2 = np.zeros(n, np.uint8)
        need2[::3] = 1
        need2[ids] |= 2
        _native.check(L.octa_sim_kat_kd_order_signflag(ctx, pts.ctypes.data, n, need2.ctypes.data, 2, out.ctypes.data), "octa_sim_kat_kd_order_signflag")
        assert sorted(out.tolist()) == list(range(n))
        got[out] = np.arange(n)
        assert (got[ids] == pos[ids]).all(), (n, ids.tolist(), "sign flag")


@pytest.mark.parametrize("name", CASES)
def test_bytes_traces_and_the_host_builds_path_counts(gh, golden, host, name):
    """The device build prints the reference's CSV bytes and per-iteration statistics (for the run across the mode switch, whose iteration
    100 replays its thousands of hits in HBM scratch: the oracle's), and takes each rung as often as the host build of the same source."""
    from oracle import sim_oracle
    seed, i1, i2, has_golden = host.CASES[name]
    sim = gh.BatchSimulator(host.config(golden, i1, i2), 1)
    res = sim.run([seed])
    assert res.stats[0, 0] == 0
    text = gh.edges_to_csv_text(res.sample_edges(0)).encode()
    trace = sim.trace()[0].copy()
    paths = tuple(int(v) for v in _kd_paths(sim, 1)[0])
    sim.close()
    if has_golden:
        assert text == golden[name + "_csv"].tobytes()
        assert (trace == golden[name + "_trace"]).all()
    else:
        e_or, info = sim_oracle.simulate(host.config(golden, i1, i2), seed)
        assert text == sim_oracle.edges_to_csv_text(e_or).encode()
        assert (trace == info["trace"]).all()
    want = host.host_run(host.load("libkdpartialhost_plain.so", []), golden, name)[2]
    print(f"{name}: device certified / partial / full {paths}; host {want}")
    assert paths[1] > 0 and paths == want


def test_full_occupancy_short_launch_is_deterministic(gh, golden, host):
    """Two samples per CU (the group flags and the need bits are HBM scratch handed over behind barriers): one launch of the 30 + 20
    configuration run twice on the same seeds gives the same per-iteration statistics, doubles and path counts."""
    import torch
    n = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    seeds = list(range(n))
    sim = gh.BatchSimulator(host.config(golden, 30, 20), n)
    res = sim.run(seeds)
    assert int(res.stats[:, 0].max()) == 0
    assert gh.edges_to_csv_text(res.sample_edges(0)).encode() == golden["run_s0_30_20_csv"].tobytes()
    trace, edges, paths = sim.trace().copy(), res.edges.copy(), _kd_paths(sim, n)
    res = sim.run(seeds)
    assert int(res.stats[:, 0].max()) == 0
    bad = np.flatnonzero((sim.trace() != trace).any(axis=(1, 2)))
    assert bad.size == 0, f"per-iteration statistics of samples {bad[:8].tolist()} differ between two runs"
    assert res.edges.shape == edges.shape and (res.edges == edges).all()
    assert (_kd_paths(sim, n) == paths).all() and (paths[:, 1] > 0).all()
