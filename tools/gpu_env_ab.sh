#!/bin/bash
# Headline bench A/B/A/B of an environment switch: bash tools/gpu_env_ab.sh TAG VAR VAL_A VAL_B
OUT=${OUT:-bench_out}   # where the logs and result lines go
set -o pipefail
mkdir -p $OUT
for r in 1 2; do
  for v in $3 $4; do
    env $2=$v timeout -k 10 300 python bench.py --full --steps 2 --no-cpu --no-train --no-e2e --no-fusion > $OUT/$1_${v}_$r.json 2> $OUT/$1_${v}_$r.err || exit 1
  done
done
