#!/bin/bash
# rocprofv3 kernel traces of decode (eager timing pass: bench.py --roofline-only) for the given configs
REPO=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$REPO/bench_out}  # where this script writes; override with OUT=...
mkdir -p "$OUT"
cd $REPO && mkdir -p $OUT
O=$OUT
cd /tmp && export TMPDIR=/tmp
for c in "$@"; do
  timeout -k 10 300 rocprofv3 --kernel-trace -d $O/trace_$c -o run --output-format csv -- \
    python3 $REPO/bench.py --full --config $c --roofline-only --timing-steps 4 --warmup 0 --pipe-stages 0 --skip-cpu \
    > $O/trace_$c.log 2>&1 || { tail -5 $O/trace_$c.log; exit 1; }
done
echo done
