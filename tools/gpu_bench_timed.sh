#!/bin/bash
# The complete bench command (bench.py --full), timed, into $OUT/$1.json (+ wall seconds in $1.time)
OUT=${OUT:-bench_out}   # where the logs and result lines go
set -o pipefail
mkdir -p $OUT
s=$(date +%s)
timeout -k 10 1000 python bench.py --full > $OUT/$1.json 2> $OUT/$1.err || exit 1
echo $(( $(date +%s) - s )) > $OUT/$1.time
