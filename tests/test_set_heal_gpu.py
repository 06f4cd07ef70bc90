"""GPU: the healing rule of the set-order certificates (phase_satisfy_art, csrc/sim_core.h) in the device build, where the whole workgroup
evaluates a pending range's verdict behind each table generation's priority insertion: the reference's bytes on the short fixtures, the
oracle's doubles across the mode switch (iteration 100 replays its thousands of hits in HBM scratch), the same three path counts
(certified / partial kd order / full kd order) as the host build of the same source, and run-to-run equality of a small batch."""
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


@pytest.fixture(scope="module")
def host_lib(host):
    return host.load("libsethealhost_heal.so", [])


def _kd_paths(sim, n):
    from octa_autosegmentation_amd import _native
    paths = np.zeros((n, 3), np.int64)
    _native.check(sim._lib.octa_sim_kd_paths(sim._h, paths.ctypes.data), "octa_sim_kd_paths")
    return paths


@pytest.mark.parametrize("name", CASES)
def test_bytes_traces_and_the_host_builds_path_counts(gh, golden, host, host_lib, name):
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
    want = host.host_run(host_lib, golden, name)[2]
    print(f"{name}: device certified / partial / full {paths}; host {want}")
    assert paths == want


def test_a_batch_of_eight_short_samples_is_deterministic_and_counts_like_the_host(gh, golden, host, host_lib):
    """Eight samples of the 30 + 20 configuration in one launch of the default build (two workgroups per CU), run twice: equal edges,
    per-iteration statistics and path counts; samples 0 and 3 are the fixtures."""
    seeds = list(range(8))
    sim = gh.BatchSimulator(host.config(golden, 30, 20), 8)
    res = sim.run(seeds)
    assert int(res.stats[:, 0].max()) == 0
    assert gh.edges_to_csv_text(res.sample_edges(0)).encode() == golden["run_s0_30_20_csv"].tobytes()
    assert gh.edges_to_csv_text(res.sample_edges(3)).encode() == golden["run_s3_30_20_csv"].tobytes()
    trace, edges, paths = sim.trace().copy(), res.edges.copy(), _kd_paths(sim, 8)
    res = sim.run(seeds)
    assert int(res.stats[:, 0].max()) == 0
    assert (sim.trace() == trace).all()
    assert res.edges.shape == edges.shape and (res.edges == edges).all()
    assert (_kd_paths(sim, 8) == paths).all()
    sim.close()
    for s, name in ((0, "run_s0_30_20"), (3, "run_s3_30_20")):
        assert tuple(int(v) for v in paths[s]) == host.host_run(host_lib, golden, name)[2]
