#!/bin/bash
# Quick GPU cycle on the box: parity tests, then a rocprofv3 kernel trace of a short bench run.
# Usage: tools/gpu_quick.sh TAG [skip-tests]
REPO=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$REPO/bench_out}  # where this script writes; override with OUT=...
mkdir -p "$OUT"
TAG=${1:-x}
cd $REPO
if [ "$2" != "skip-tests" ]; then
  timeout -k 10 300 python -u -m pytest tests -m gpu -q -p no:cacheprovider --timeout 120 --timeout-method thread -x > $OUT/gpu_$TAG.log 2>&1
  rc=$?
  echo EXIT $rc >> $OUT/gpu_$TAG.log
  if [ $rc -ne 0 ]; then exit $rc; fi
fi
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv -- python3 $REPO/bench.py --full --steps 64 --skip-cpu --seq-reps 1 > $OUT/prof_$TAG.log 2>&1
