#!/bin/bash
# rocprofv3 kernel stats of one BASELINE configuration's bench (decode + sequence eval).
# Usage: tools/prof_cfg2.sh CONFIG TAG
REPO=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$REPO/bench_out}  # where this script writes; override with OUT=...
mkdir -p "$OUT"
ROOT=$REPO
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_$2 -o run --output-format csv -- \
  python3 $ROOT/bench.py --full --config $1 --steps 32 --skip-cpu --seq-reps 2 --batch "" --abi-steps 0 > $OUT/prof_$2.log 2>&1 || { tail -5 $OUT/prof_$2.log; exit 5; }
grep -E "decode:|seq-eval" $OUT/prof_$2.log
python3 $ROOT/tools/top_kernels.py $OUT/prof_$2/run_kernel_stats.csv 26
