"""What the on-chip sink sampling (csrc/sim_core.h: phase_sample) does per call, counted on the CPU: the host build of the phase code
with -DOCTA_SIM_SAMPLE_COUNT, full-length samples of the generator configuration. usage: python tools/sample_counts.py [seed ...]
(add -DOCTA_SIM_SAMPLE_NODE_FIRST=1 through OCTA_COUNT_FLAGS to count the other pass order). Counts, not times."""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from octa_autosegmentation_amd.utils import configs  # noqa: E402
from oracle import sim_oracle  # noqa: E402

NAMES = ["calls", "candidates", "valid", "arterial nodes", "live sinks", "slots seen by the sink pass", "... live", "slots seen by the node pass", "... live",
         "live between the passes", "passers", "accepted"]


def main():
    seeds = [int(a) for a in sys.argv[1:]] or [5000]
    flags = os.environ.get("OCTA_COUNT_FLAGS", "").split()
    so = os.path.join(ROOT, "tests", "native", "libsampleonchip_count.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-fPIC", "-shared", "-DOCTA_SIM_SAMPLE_COUNT"] + flags +
                          ["-o", so, os.path.join(ROOT, "tests", "native", "sample_onchip_host.cpp")])
    lib = ctypes.CDLL(so)
    lib.octa_simcore_host_run.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_ulonglong, sim_oracle.BIF_CB, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p]
    lib.octa_sample_counts.argtypes = [ctypes.c_void_p, ctypes.c_int]
    cfg = configs.load_generator_config()
    p = sim_oracle.params_from_config(cfg)
    for seed in seeds:
        edges = np.zeros((200000, 7)); trace = np.zeros((1000, 4), np.int64); info = np.zeros(8, np.int64)
        rc = lib.octa_simcore_host_run(ctypes.addressof(p), seed, seed, sim_oracle._bif_cb, edges.ctypes.data, len(edges), trace.ctypes.data, info.ctypes.data)
        assert rc == 0, rc
        c = np.zeros(12, np.int64)
        lib.octa_sample_counts(c.ctypes.data, 1)
        print(f"seed {seed}: {c[0]} calls; per call: " + ", ".join(f"{n} {v / c[0]:.1f}" for n, v in zip(NAMES[1:], c[1:])))


if __name__ == "__main__":
    main()
