#!/bin/bash
# Round-3 measurement cycle on the GPU box: GPU tests, smoke, the default bench line and the
# rocprofv3 kernel-trace stats of the bench workload.  Every GPU step has its own time limit;
# the script stops at the first failure.  Usage: tools/r3_cycle.sh TAG [tests|notests]
REPO=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$REPO/bench_out}  # where this script writes; override with OUT=...
mkdir -p "$OUT"
TAG=${1:-r3}
MODE=${2:-tests}
ROOT=$REPO
cd $ROOT
mkdir -p $OUT
if [ "$MODE" = tests ]; then
  timeout -k 10 700 python3 -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/${TAG}_gputest.log 2>&1 || { tail -30 $OUT/${TAG}_gputest.log; exit 1; }
  tail -3 $OUT/${TAG}_gputest.log
  timeout -k 10 120 python3 -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1 || { cat $OUT/${TAG}_smoke.log; exit 1; }
  tail -1 $OUT/${TAG}_smoke.log
fi
timeout -k 10 400 python3 bench.py --full > $OUT/${TAG}_bench.log 2>&1 || { tail -15 $OUT/${TAG}_bench.log; exit 1; }
grep '^{' $OUT/${TAG}_bench.log > $OUT/${TAG}_bench.json
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG} -o run --output-format csv -- \
  python3 $ROOT/bench.py --full --steps 64 --skip-cpu --seq-reps 1 --batch 8 --abi-steps 4 > $OUT/prof_${TAG}.log 2>&1 || { tail -5 $OUT/prof_${TAG}.log; exit 1; }
echo done
