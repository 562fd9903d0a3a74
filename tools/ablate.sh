#!/bin/bash
# Ablation builds of the trace kernels: what does each part of the ray body cost?  (diagnostic libraries only: results are wrong;
# the switches live in artist_amd/csrc/trace_diag.hpp; "base" is the product library)
# usage: bash tools/ablate.sh build   (anywhere)   |   bash tools/ablate.sh run   (GPU box; prints fwd/bwd ms per variant)
set -eo pipefail   # a bench run that fails, faults or runs into its limit ends the script: nothing more is started on the GPU
cd "$(dirname "$0")/.."
VARIANTS="noatomics:-DART_ABLATE_NO_LDS_ATOMICS nostrays:-DART_ABLATE_NO_STRAYS noloads:-DART_ABLATE_NO_LOADS noflush:-DART_ABLATE_NO_FLUSH aluonly:-DART_ABLATE_NO_LDS_ATOMICS,-DART_ABLATE_NO_STRAYS,-DART_ABLATE_NO_LOADS"
if [ "$1" = build ]; then
  for v in $VARIANTS; do
    name=${v%%:*}; defs=$(echo ${v#*:} | tr ',' ' ')
    make -C artist_amd/csrc -j16 DIAG="$defs" OBJDIR=../../tools/bin/obj_$name OUT=../../tools/bin/libdiag_$name.so
  done
  exit 0
fi
for v in base $VARIANTS; do
  name=${v%%:*}
  if [ $name = base ]; then unset ARTIST_HIP_LIB; else export ARTIST_HIP_LIB=$PWD/tools/bin/libdiag_$name.so; fi
  out=$(timeout -k 10 200 python bench.py --steps 5 --warmup 2 --full --no-cpu-baseline --no-check "${@:2}" 2>/dev/null) || exit 1
  ms=$(tail -1 <<<"$out" | python -c 'import sys,json; d=json.loads(sys.stdin.read()); k=d["kernels"]; print("fwd %.3f ms  bwd %.3f ms" % (k["trace_fwd_ms"], k["trace_bwd_ms"]))') || exit 1
  echo "$name $ms"
done
