#!/bin/bash
# rocprofv3 kernel trace of a few decode tokens (no timing pass) -- tools/, on the GPU box
REPO=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$REPO/bench_out}  # where this script writes; override with OUT=...
mkdir -p "$OUT"
TAG=${1:-dec}
cd /tmp && export TMPDIR=/tmp
timeout -k 10 200 rocprofv3 --kernel-trace -d $OUT/tr_$TAG -o run --output-format csv -- \
  python3 $REPO/bench.py --full --steps 8 --warmup 2 --batch "" --seq-reps 0 --abi-steps 0 --skip-cpu --timing-steps 1 \
  > $OUT/tr_$TAG.log 2>&1
