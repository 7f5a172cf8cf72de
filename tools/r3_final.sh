#!/bin/bash
# End-of-round-3 cycle at the final HEAD: GPU tests, smoke, bench line, rocprof stats (r3_cycle.sh),
# then the other BASELINE configurations' bench lines (decode, seq-eval, B = 8 / 64 batched).
REPO=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$REPO/bench_out}  # where this script writes; override with OUT=...
mkdir -p "$OUT"
cd $REPO && mkdir -p $OUT
TAG=${1:-r3d}
bash tools/r3_cycle.sh $TAG tests || exit 1
grep -E "decode|seq-eval" $OUT/${TAG}_bench.log | cut -c1-160
for c in v4-169m-q8_0 v7-2b9-q5_1 v5-7b-q4_1; do
  timeout -k 10 400 python3 bench.py --full --config $c --steps 64 --warmup 8 --batch "8,64" --seq-reps 2 --abi-steps 8 --skip-cpu > $OUT/${TAG}_$c.log 2>&1 || { tail -5 $OUT/${TAG}_$c.log; exit 1; }
  grep '^{' $OUT/${TAG}_$c.log > $OUT/${TAG}_$c.json
  grep -E "decode|seq-eval" $OUT/${TAG}_$c.log | sed "s/^/[$c] /" | cut -c1-160
done
echo done
