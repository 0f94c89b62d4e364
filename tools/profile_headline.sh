#!/bin/bash
# The headline bench with everything it reports (--full: the CPU baseline and the parity on its
# sample), then its rocprofv3 kernel stats.  Usage on the GPU box: bash tools/profile_headline.sh [OUT_DIR]
cd "$(dirname "$0")/.." || exit 1
export TMPDIR=/tmp
O=${1:-bench_out/headline}; mkdir -p "$O"
timeout -k 10 120 python -m pytest tests/test_gpu_freegas.py -x -q -m gpu -k "task_order" > "$O/t.log" 2>&1 || { tail -20 "$O/t.log"; exit 1; }
timeout -k 10 400 python bench.py --full > "$O/bench_default.json" 2> "$O/bench_default.err" || exit 1
rm -rf "$O/prof"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/prof" -- python bench.py --steps 2 --warmup 1 > "$O/bench_rocprof.json" 2> "$O/bench_rocprof.err" || exit 1
tail -1 "$O/t.log"; tail -c 1500 "$O/bench_default.json"
