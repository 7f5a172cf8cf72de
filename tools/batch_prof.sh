#!/bin/bash
# rocprofv3 kernel summary of the batched decode (B contexts per step) -- tools/, run on the GPU box
REPO=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$REPO/bench_out}  # where this script writes; override with OUT=...
mkdir -p "$OUT"
B=${1:-8}
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_batch$B -o run --output-format csv -- \
  python3 $REPO/bench.py --full --steps 4 --warmup 2 --batch $B --batch-steps 20 --seq-reps 0 --abi-steps 0 \
  --skip-cpu --timing-steps 1 > $OUT/prof_batch$B.log 2>&1
