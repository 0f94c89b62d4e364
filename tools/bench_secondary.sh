#!/bin/bash
# Runs every secondary bench workload once with the CPU port beside it (--full; JSON lines ->
# OUT_DIR/kernels/), then rocprofv3 kernel stats of the heavier ones.
# Usage on the GPU box: bash tools/bench_secondary.sh [OUT_DIR]
set -e
cd "$(dirname "$0")/.."
O=${1:-bench_out}/kernels
mkdir -p "$O"
for w in file4 file6cm file6cm_g70 file6lab file6lab_g70 law9 sab_disc sab_cont chi; do
  timeout -k 10 300 python3 bench.py --workload $w --full --steps 3 --warmup 1 > "$O/$w.json" 2> "$O/$w.err"
  cut -c1-400 "$O/$w.json"
done
export TMPDIR=/tmp
for w in file4 file6cm_g70 file6lab_g70; do
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/prof_$w" -o $w -- python3 bench.py --workload $w --steps 3 --warmup 1 > "$O/prof_$w.log" 2>&1
done
ls "$O"
