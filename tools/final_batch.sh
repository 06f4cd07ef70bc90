#!/bin/bash
# The closing measurements of a round in one GPU session, logs under DIR. Every step runs under its own time limit, and the batch stops
# at the first step that fails (a time limit, an abort or a fault included): nothing more is started on the GPU after it. The scripts
# it runs stop at their own first failed command (bash -e -o pipefail).
# usage: bash tools/final_batch.sh DIR
set -o pipefail
out=$(mkdir -p "${1:?usage: tools/final_batch.sh DIR}" && cd "$1" && pwd) || exit 1
cd "$(dirname "$0")/.." || exit 1
timeout -k 10 2000 bash -e -o pipefail tools/profile_bench.sh r06 "$out" > "$out"/profile_bench.log 2>&1 \
&& timeout -k 10 1300 bash -e -o pipefail tools/raster_pmc.sh r06 > "$out"/raster_pmc.log 2>&1 \
&& { timeout -k 10 1800 python tools/sim_counters.py 2>&1 | grep -v amdgpu | tail -34 > "$out"/sim_counters.log; } \
&& timeout -k 10 4000 bash -e -o pipefail tools/sim_check.sh final2 tests 30 > "$out"/sim_check_final2.log 2>&1 \
&& timeout -k 10 900 python bench.py --gpus 1 --steps 20 --warmup 5 --full > "$out"/bench_final.json 2> "$out"/bench_final.err
rc=$?
[ $rc -eq 0 ] || { echo "final_batch: stopped at a failed step (exit status $rc)"; exit $rc; }
python tools/bench_line.py value value_with_csv roofline.avg_launch_ms roofline.frac roofline.traffic unet_train.value end_to_end_train.value end_to_end_gan_seg_train.value end_to_end_10k_epoch.value train_cli.value cpu_baseline.value mailbox.relaunches < "$out"/bench_final.json
tail -3 "$out"/sim_check_final2.log
