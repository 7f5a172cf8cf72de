#!/bin/bash
# Decode roofline reproducibility: the bench line (per-dispatch event roofline), then a rocprofv3
# kernel trace of `bench.py --decode-only` (graph-replayed decode only), then the recompute of the
# line's roofline from that trace.  Usage: tools/r4_prof.sh TAG
REPO=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$REPO/bench_out}  # where this script writes; override with OUT=...
mkdir -p "$OUT"
TAG=${1:-p}
ROOT=$REPO
cd $ROOT && mkdir -p $OUT
timeout -k 10 300 python3 bench.py --full --skip-cpu --batch "" --seq-reps 1 --abi-steps 4 > $OUT/${TAG}_line.log 2>&1 || { tail -5 $OUT/${TAG}_line.log; exit 1; }
grep -E "decode:" $OUT/${TAG}_line.log
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG} -o run --output-format csv -- \
  python3 $ROOT/bench.py --decode-only --steps 256 > $OUT/prof_${TAG}.log 2>&1 || { tail -5 $OUT/prof_${TAG}.log; exit 1; }
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/profr_${TAG} -o run --output-format csv -- \
  python3 $ROOT/bench.py --full --roofline-only --timing-steps 32 --warmup 0 > $OUT/profr_${TAG}.log 2>&1 || { tail -5 $OUT/profr_${TAG}.log; exit 1; }
cd $ROOT
CSV=$(find $OUT/prof_${TAG} -name "*kernel_stats.csv" | head -1)
echo "stats: $CSV"
python3 tools/roofline_from_csv.py $CSV $OUT/${TAG}_line.log | tee $OUT/${TAG}_roofline_check.json

CSV2=$(find $OUT/profr_${TAG} -name "*kernel_stats.csv" | head -1)
echo "roofline-pass stats: $CSV2"
python3 tools/roofline_from_csv.py $CSV2 $OUT/profr_${TAG}.log | tee $OUT/${TAG}_roofline_check_eager.json
echo done
