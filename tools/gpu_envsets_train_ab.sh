#!/bin/bash
# Headline bench with the training section under several environment sets, twice in turn:
# bash tools/gpu_envsets_train_ab.sh TAG "A=1" "A=0" ...  -> $OUT/TAG_<i>_<r>.json
OUT=${OUT:-bench_out}   # where the logs and result lines go
set -o pipefail
mkdir -p $OUT
tag=$1; shift
for r in 1 2; do
  i=0
  for set in "$@"; do
    env $set timeout -k 10 400 python bench.py --full --steps 2 --no-cpu --no-e2e --no-fusion > $OUT/${tag}_${i}_$r.json 2>/dev/null || exit 1
    i=$((i+1))
  done
done
