#!/bin/bash
# The complete bench line (bench.py --full, every leg) into $OUT/$1.json
OUT=${OUT:-bench_out}   # where the logs and result lines go
set -o pipefail
mkdir -p $OUT
timeout -k 10 1000 python bench.py --full > $OUT/$1.json 2> $OUT/$1.err
