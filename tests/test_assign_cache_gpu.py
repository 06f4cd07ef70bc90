"""GPU: phase_assign's memory of each attractor's nearest active node (csrc/sim_core.h) in the device build: the reference's bytes on
the two short fixtures of tests/test_assign_cache.py, the same path per attractor as the host build, and run-to-run equality with two
samples per CU."""
import os

import numpy as np
import pytest
import yaml

pytestmark = pytest.mark.gpu

CASES = ("run_s0_30_20", "run_s11_20_0")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "sim_golden.npz"))


@pytest.fixture(scope="module")
def gh(hip_lib_built):
    import torch
    assert torch.cuda.is_available()
    from octa_autosegmentation_amd.vessel_graph_generation import greenhouse
    return greenhouse


def _cfg(golden, i1, i2):
    cfg = yaml.safe_load(str(golden["config_yaml"]))
    cfg["Greenhouse"]["modes"][0]["I"] = int(i1)
    cfg["Greenhouse"]["modes"][1]["I"] = int(i2)
    return cfg


def _assign_paths(sim, n):
    from octa_autosegmentation_amd import _native
    paths = np.zeros((n, 2), np.int64)
    _native.check(sim._lib.octa_sim_assign_paths(sim._h, paths.ctypes.data), "octa_sim_assign_paths")
    return paths


@pytest.mark.parametrize("name", CASES)
def test_short_fixture_bytes_and_the_host_builds_paths(gh, golden, name):
    """The device build prints the reference's CSV bytes and per-iteration statistics, and answers as many attractors incrementally /
    by the grid scan as the host build of the same source does for the same seed."""
    import test_assign_cache as host
    seed, i1, i2 = (int(v) for v in golden[name + "_seed_I"])
    sim = gh.BatchSimulator(_cfg(golden, i1, i2), 1)
    res = sim.run([seed])
    assert res.stats[0, 0] == 0
    assert gh.edges_to_csv_text(res.sample_edges(0)).encode() == golden[name + "_csv"].tobytes()
    assert (sim.trace()[0] == golden[name + "_trace"]).all()
    inc, full = (int(v) for v in _assign_paths(sim, 1)[0])
    sim.close()
    info = host.host_run(host._load("libassigncachehost_shipped.so", []), golden, name)[2]
    print(f"{name}: device {inc} incremental / {full} by the grid scan; host {int(info[8])} / {int(info[9])}")
    assert inc > 0 and (inc, full) == (int(info[8]), int(info[9]))


def test_full_occupancy_short_launch_is_deterministic(gh, golden):
    """Two samples per CU (the memory is cross-phase state in HBM, its staging area shares the LDS with the grid): one launch of the
    short configuration run twice on the same seeds gives the same per-iteration statistics and the same doubles, and seed 0 among
    them the reference's bytes."""
    import torch
    name = "run_s0_30_20"
    n = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    seeds = list(range(n))
    sim = gh.BatchSimulator(_cfg(golden, 30, 20), n)
    res = sim.run(seeds)
    assert int(res.stats[:, 0].max()) == 0
    assert gh.edges_to_csv_text(res.sample_edges(0)).encode() == golden[name + "_csv"].tobytes()
    trace, edges, paths = sim.trace().copy(), res.edges.copy(), _assign_paths(sim, n)
    res = sim.run(seeds)
    assert int(res.stats[:, 0].max()) == 0
    bad = np.flatnonzero((sim.trace() != trace).any(axis=(1, 2)))
    assert bad.size == 0, f"per-iteration statistics of samples {bad[:8].tolist()} differ between two runs"
    assert res.edges.shape == edges.shape and (res.edges == edges).all()
    assert (_assign_paths(sim, n) == paths).all() and (paths[:, 0] > 0).all()
    sim.close()
