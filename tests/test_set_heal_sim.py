"""CPU: the healing rule of the set-order certificates inside the O2 -> CO2 conversion (phase_satisfy_art, csrc/sim_core.h), on the host
build of the phase code (tests/native/kd_partial_host.cpp): the default build (violations of a table generation that is resized stay
pending for the next generation's verdict) and -DOCTA_SIM_SET_NOHEAL (the strict certificates, the A/B partner) on the cases of
tests/test_kd_partial.py. Both must print the reference's bytes where fixtures exist and equal the oracle in every double and every
per-iteration statistic; the default certifies at least as many conversions and builds at most as many kd orders."""
import pytest

import test_kd_partial as host

BUILDS = {"heal": [], "strict": ["-DOCTA_SIM_SET_NOHEAL"]}


@pytest.fixture(scope="module")
def golden():
    return host.np.load(host.os.path.join(host.ROOT, "tests", "golden", "sim_golden.npz"))


@pytest.fixture(scope="module")
def oracle_runs(golden):
    out = {}
    for name, (seed, i1, i2, _) in host.CASES.items():
        edges, info = host.sim_oracle.simulate(host.config(golden, i1, i2), seed)
        out[name] = (edges, info["trace"])
    return out


@pytest.fixture(scope="module")
def runs(golden):
    libs = {k: host.load(f"libsethealhost_{k}.so", flags) for k, flags in BUILDS.items()}
    return {(k, name): host.host_run(lib, golden, name) for k, lib in libs.items() for name in host.CASES}


@pytest.mark.parametrize("name", list(host.CASES))
@pytest.mark.parametrize("build", list(BUILDS))
def test_both_builds_give_the_reference_bytes_and_the_oracles_doubles(runs, oracle_runs, golden, build, name):
    edges, trace, _ = runs[(build, name)]
    e_or, t_or = oracle_runs[name]
    assert (trace == t_or).all()
    assert e_or.shape == edges.shape and e_or.tobytes() == edges.tobytes()
    if host.CASES[name][3]:
        assert (trace == golden[name + "_trace"]).all()
        assert host.sim_oracle.edges_to_csv_text(edges).encode() == golden[name + "_csv"].tobytes()


@pytest.mark.parametrize("name", list(host.CASES))
def test_healing_certifies_no_less_and_builds_no_more_kd_orders(runs, name):
    cert, part, full = runs[("heal", name)][2]
    cert_s, part_s, full_s = runs[("strict", name)][2]
    print(f"{name}: certified / partial / full: healing {cert} / {part} / {full}, strict {cert_s} / {part_s} / {full_s}")
    assert cert + part + full == cert_s + part_s + full_s          # the same conversions
    assert cert >= cert_s
    assert part + full <= part_s + full_s
