#!/bin/bash
# Round measurements of the fp32 path (run on the GPU box from the repo root): kernel-trace stats of the bench
# command, then one rocprofv3 --pmc pass per counter set (each its own process, kernel-trace only).
set -e
export OUT=${OUT:-out}  # where every output of this script goes
mkdir -p $OUT
R=${1:-r01}
export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${R}_kt -o ${R} -- python3 bench.py --full --no-cpu-baseline --psnr-steps 0 > $OUT/${R}_kt.log 2>&1
for set in "FETCH_SIZE" "WRITE_SIZE" "SQ_INSTS_VALU_MFMA_MOPS_F32 SQ_INSTS_VALU"; do
  name=$(echo $set | cut -d' ' -f1)
  rocprofv3 --kernel-trace --output-format csv --pmc $set -d $OUT/${R}_pmc_$name -o ${R} -- python3 bench.py --full --steps 40 --warmup 5 --no-cpu-baseline --no-bf16 --psnr-steps 0 > $OUT/${R}_pmc_$name.log 2>&1
done
ls $OUT/${R}_kt $OUT/${R}_pmc_*
