#!/bin/bash
# GPU check after a change: the full GPU test suite, then a short headline bench line
# (no CPU / fusion / e2e legs).  usage: bash tools/gpu_check.sh <tag> [extra bench args]
OUT=${OUT:-bench_out}   # where the logs and result lines go
set -o pipefail
tag=${1:-chk}; shift
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread \
  > $OUT/${tag}_tests.log 2>&1; rc=$?
tail -3 $OUT/${tag}_tests.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -u bench.py --full --steps 3 --warmup 1 --no-cpu --no-fusion --no-e2e "$@" \
  > $OUT/${tag}_bench.json 2> $OUT/${tag}_bench.err; rc=$?
cut -c1-600 $OUT/${tag}_bench.json
exit $rc
