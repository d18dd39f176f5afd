#!/bin/bash
# rocprofv3 kernel statistics of the headline bench command (the roofline's kernel average
# must agree with bench.py's hipEvent figure) -> $OUT/$1/
OUT=${OUT:-bench_out}   # where the logs and result lines go
set -o pipefail
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
mkdir -p $R/$OUT
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$OUT/$1 -o run -- \
  python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu --no-train --no-e2e --no-fusion > $R/$OUT/$1.json 2> $R/$OUT/$1.err
