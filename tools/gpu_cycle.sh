#!/bin/bash
# One GPU cycle on the box: parity tests, bench (with the CPU baseline), rocprofv3 kernel trace.
# Usage: tools/gpu_cycle.sh TAG [skip-tests]
REPO=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$REPO/bench_out}  # where this script writes; override with OUT=...
mkdir -p "$OUT"
TAG=${1:-x}
cd $REPO
if [ "$2" != "skip-tests" ]; then
  timeout -k 10 600 python -u -m pytest tests -m gpu -q -p no:cacheprovider --timeout 300 --timeout-method thread -x > $OUT/gpu_$TAG.log 2>&1
  rc=$?
  echo EXIT $rc >> $OUT/gpu_$TAG.log
  # test failures (1) still allow a measurement; a fault, abort or timeout ends the call
  if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
fi
timeout -k 10 400 python bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || exit 1
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv -- python3 $REPO/bench.py --full --steps 64 --skip-cpu --seq-reps 1 > $OUT/prof_$TAG.log 2>&1
