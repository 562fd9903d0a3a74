#!/bin/bash
export ARTIST_HIP_DEBUG=1   # the library reads its ARTIST_HIP_* knobs only in debug mode
# Where does a workgroup's time go?  Builds the library with -DART_DEBUG_TIMELINE (artist_amd/csrc/trace_diag.hpp: every work
# item stamps its phases with the 100 MHz real-time counter), runs the metric field on the GPU box and prints per-phase
# medians + the gap a CU leaves between two workgroups.
# usage: bash tools/timeline.sh build   (anywhere: hipcc cross-compiles)   then, on the GPU box: bash tools/timeline.sh run [H]
set -e
cd "$(dirname "$0")/.."
if [ "$1" = build ]; then
  make -C artist_amd/csrc -j16 DIAG="-DART_DEBUG_TIMELINE $ART_EXTRA_DEFS" OBJDIR=../../tools/bin/obj_timeline OUT=../../tools/bin/libdiag_timeline.so
  exit 0
fi
H=${2:-1000}
T=${OUT:-tools_out}; mkdir -p $T
ARTIST_HIP_LIB=$PWD/tools/bin/libdiag_timeline.so ART_TIMELINE_OUT=$T/timeline.bin ART_TIMELINE_OUT_BWD=$T/timeline_bwd.bin \
  timeout -k 10 300 python bench.py --heliostats $H --steps 2 --warmup 1 --full --no-cpu-baseline --no-check > /dev/null
echo "forward:"; if [ "${ARTIST_HIP_LEAN:-1}" = 1 ]; then python tools/timeline_lean_report.py $T/timeline.bin; else python tools/timeline_report.py $T/timeline.bin; fi
echo "backward:"; python tools/timeline_report.py $T/timeline_bwd.bin
