#!/bin/bash
# MFMA-pipe utilisation of the sweep's kernels (rocprofv3 PMC pass, 8 planes of the headline
# sweep, serialised kernel-timing pass included): SQ_VALU_MFMA_BUSY_CYCLES, SQ_BUSY_CYCLES,
# GRBM_GUI_ACTIVE, SQ_INSTS_VALU, SQ_INSTS_MFMA
OUT=${OUT:-bench_out}   # where the logs and result lines go
set -o pipefail
export TMPDIR=/tmp
mkdir -p $OUT
rm -rf $OUT/pmc_mfma
timeout -s KILL 180 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_INSTS_VALU SQ_INSTS_MFMA \
  --output-format csv -d $OUT/pmc_mfma -o m -- python bench.py --full --no-cpu --no-fusion --no-e2e --no-train --planes 8 \
  --steps 1 --warmup 0 > $OUT/pmc_mfma.log 2>&1 || { tail -5 $OUT/pmc_mfma.log; exit 1; }
python tools/pmc_show.py $OUT/pmc_mfma lstm omega cost_x deconv head
