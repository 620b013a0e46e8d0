#!/bin/bash
# Kernel durations of the bf16 path from rocprofv3 (run on the GPU box from the repo root): tools/prof_bf16.sh TAG [B ...]
set -o pipefail
export OUT=${OUT:-out}  # where every output of this script goes
mkdir -p $OUT
R=${1:-bf16}; shift
export TMPDIR=/tmp
ROOT=$(pwd)
(cd /tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $ROOT/$OUT/${R}_kt -o ${R} -- python3 $ROOT/tools/bench_bf16.py "$@" > $ROOT/$OUT/${R}_kt.log 2>&1) || { echo "kernel-trace pass failed"; tail -5 $OUT/${R}_kt.log; exit 1; }
kt=$(find $OUT/${R}_kt -name '*kernel_trace.csv' | head -1)
python3 tools/kernel_stats_by_grid.py "$kt" > $OUT/${R}_kernel_stats_by_grid.csv
rm -rf $OUT/${R}_kt
cat $OUT/${R}_kernel_stats_by_grid.csv | cut -c1-200 | head -20
tail -2 $OUT/${R}_kt.log
