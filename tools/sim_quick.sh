#!/bin/bash
# Quick simulator check on the GPU box: parity tests of the simulator + the headline bench leg with the rasteriser timed alone and the
# counter passes (bench.py --full without the CPU baseline / files / training legs). Each step runs under its own time limit; the
# bench starts only when the tests passed.
# usage: tools/sim_quick.sh TAG OUT_DIR
set -o pipefail
tag=${1:?usage: tools/sim_quick.sh TAG OUT_DIR}
out=${2:?usage: tools/sim_quick.sh TAG OUT_DIR}
mkdir -p "$out" || exit 1
timeout -k 10 1500 python -m pytest tests/test_sim_gpu.py tests/test_fullsize_gpu.py -q -m gpu -x -k "not voxel and not dynunet and not unet and not conv" 2>&1 | tail -5 > "$out"/${tag}_tests.log
rc=$?
cat "$out"/${tag}_tests.log
[ $rc -eq 0 ] || { echo "sim_quick: the tests failed (exit status $rc); the bench is not started"; exit $rc; }
timeout -k 10 900 python bench.py --full --no-cpu-baseline --no-train --no-end-to-end --no-files > "$out"/${tag}_bench.json 2> "$out"/${tag}_bench.err || exit $?
python - <<PY
import json
d = json.loads(open("$out/${tag}_bench.json").read().strip().splitlines()[-1])
r = d["roofline"]
print("samples/s", round(d["value"], 1), "ms/step", round(d["ms_per_step"], 1), "launch ms", round(r["avg_launch_ms"], 1),
      "per-sample ms", round(r["serial_depth"]["per_sample_device_ms"], 1), "solo launch", round(r["serial_depth"]["solo_launch_ms"], 1))
print({k: v for k, v in r["serial_depth"].items() if "phase" in k or "ms" in k})
PY
