#!/bin/bash
# Build the in-tree sources into tools/ab/lib_NAME.so for A/B runs with AARMVS_LIB (the in-tree
# library is left as it was), optionally with extra flags for named units.  The recipe is
# csrc/Makefile's; only the object directory, the output and EXTRA_<unit> are set here.
#   bash tools/lib_variant.sh NAME [UNIT=FLAGS ...]
#   bash tools/lib_variant.sh tw32 cost_fwd=-DAARMVS_OMEGA_TW=32
#   bash tools/lib_variant.sh v cost_bwd="-DAARMVS_CBF_MINB=1 -DAARMVS_COH=1" convlstm=-DAARMVS_C3DB=0
set -eu
root="$(cd "$(dirname "$0")/.." && pwd)"
name=$1; shift
args=()
for kv in "$@"; do
  unit=${kv%%=*}
  [ -f "$root/aa-rmvsnet_amd/csrc/$unit.hip" ] || { echo "no unit $unit.hip" >&2; exit 2; }
  args+=("EXTRA_$unit=${kv#*=}")
done
make -s -C "$root/aa-rmvsnet_amd/csrc" -j"${JOBS:-8}" OBJDIR="$root/tools/ab/build_$name" \
  OUT="$root/tools/ab/lib_$name.so" ${args[@]+"${args[@]}"}
echo "built tools/ab/lib_$name.so ($*)"
