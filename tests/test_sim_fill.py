"""CPU: the simulator's threaded per-batch set-up (csrc/sim_host.h: fill_samples) on the host (tests/native/sim_fill_host.cpp). Whatever the
number of threads, the staged bytes -- scalars, generator states, valid-voxel lists, counts, stump nodes -- must be the same, and for one
sample they must be what init_sample gives directly. Batch sizes: 1; 63 and 64 (the pool starts a second thread at 64); 70 (an uneven last
range); 129 (more than two ranges when the thread knob allows it)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import yaml

from oracle import sim_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = "run_s11_20_0"          # the smallest golden configuration
BATCHES = (1, 63, 64, 70, 129)


@pytest.fixture(scope="module")
def lib():
    """(tests/test_sim_core.py: _load_core, for this file's harness)"""
    src = os.path.join(ROOT, "tests", "native", "sim_fill_host.cpp")
    so = os.path.join(ROOT, "tests", "native", "libsimfillhost.so")
    deps = [src] + [os.path.join(ROOT, "octa_autosegmentation_amd", "csrc", f) for f in ("sim_core.h", "sim_host.h", "gpow.h", "glibc_pow_tables.h", "glibc_trig.h", "glibc_trig_tables.h")]
    if not os.path.exists(so) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-o", so, src])
    l = ctypes.CDLL(so)
    l.octa_simfill_bytes.restype = ctypes.c_long
    l.octa_simfill_bytes.argtypes = [ctypes.c_void_p, ctypes.c_int]
    l.octa_simfill_run.restype = ctypes.c_int
    l.octa_simfill_run.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_ulonglong, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    l.octa_simfill_direct.restype = ctypes.c_int
    l.octa_simfill_direct.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_ulonglong, ctypes.c_void_p]
    return l


@pytest.fixture(scope="module")
def case():
    golden = np.load(os.path.join(ROOT, "tests", "golden", "sim_golden.npz"))
    seed, i1, i2 = (int(v) for v in golden[CASE + "_seed_I"])
    cfg = yaml.safe_load(str(golden["config_yaml"]))
    cfg["Greenhouse"]["modes"][0]["I"] = i1
    cfg["Greenhouse"]["modes"][1]["I"] = i2
    return sim_oracle.params_from_config(cfg), seed


def fill(lib, p, seed, B, threads, monkeypatch):
    monkeypatch.setenv("OCTA_SIM_INIT_THREADS", str(threads))
    out = np.zeros(lib.octa_simfill_bytes(ctypes.addressof(p), B), np.uint8)
    knob = ctypes.c_int(0)
    bad = lib.octa_simfill_run(ctypes.addressof(p), B, seed, seed, out.ctypes.data, ctypes.byref(knob))
    assert bad == -1, f"sample {bad} has no valid voxel"
    assert knob.value == threads
    return out


@pytest.mark.parametrize("B", BATCHES)
def test_thread_ranges_stage_the_same_bytes(lib, case, B, monkeypatch):
    p, seed = case
    one = fill(lib, p, seed, B, 1, monkeypatch)
    four = fill(lib, p, seed, B, 4, monkeypatch)
    assert one.any() and one.tobytes() == four.tobytes()


def test_one_sample_is_what_init_sample_gives(lib, case, monkeypatch):
    p, seed = case
    direct = np.zeros(lib.octa_simfill_bytes(ctypes.addressof(p), 1), np.uint8)
    assert lib.octa_simfill_direct(ctypes.addressof(p), seed, seed, direct.ctypes.data) == -1
    for threads in (1, 4):
        assert fill(lib, p, seed, 1, threads, monkeypatch).tobytes() == direct.tobytes()
    # ... and every sample of a batch is the one-sample set-up of its own seed: sample 69 of 70 (the last of the second range)
    full = fill(lib, p, seed, 70, 4, monkeypatch)
    last = np.zeros_like(direct)
    assert lib.octa_simfill_direct(ctypes.addressof(p), seed + 69, seed + 69, last.ctypes.data) == -1
    vs = 76 * 76 * 3 * 2
    assert full[69 * vs: 70 * vs].tobytes() == last[:vs].tobytes()
