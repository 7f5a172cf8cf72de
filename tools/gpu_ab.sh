#!/bin/bash
# GPU cycle used while tuning: parity tests, a short bench line, and a rocprofv3 kernel-trace of
# the sequence eval + single decode (no batched decode).  Every GPU step has its own time limit and
# the first failure ends the call.   Usage: tools/gpu_ab.sh TAG [skip-tests] [skip-prof]
REPO=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$REPO/bench_out}  # where this script writes; override with OUT=...
mkdir -p "$OUT"
TAG=${1:-x}
ROOT=$REPO
cd $ROOT
mkdir -p $OUT
if [ "$2" != "skip-tests" ]; then
  timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread > $OUT/gpu_$TAG.log 2>&1
  rc=$?
  tail -3 $OUT/gpu_$TAG.log
  if [ $rc -ne 0 ]; then grep -E "FAILED|Error|assert" $OUT/gpu_$TAG.log | head -30; exit $rc; fi
fi
timeout -k 10 300 python bench.py --full --steps 64 --warmup 8 --skip-cpu --seq-reps 3 --abi-steps 4 > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { tail -5 $OUT/bench_$TAG.err; exit 4; }
grep -E "decode:|seq-eval|k_mv |seq GEMM|batch" $OUT/bench_$TAG.err
if [ "$3" != "skip-prof" ]; then
  cd /tmp && export TMPDIR=/tmp
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv -- \
    python3 $ROOT/bench.py --full --steps 32 --skip-cpu --seq-reps 2 --batch "" --abi-steps 0 > $OUT/prof_$TAG.log 2>&1 || exit 5
  python3 $ROOT/tools/top_kernels.py $OUT/prof_$TAG/run_kernel_stats.csv
fi
echo done
