#!/bin/bash
# usage: [SRC=copy.hip] bash tools/build_obj_variant.sh FILE NAME [-DFLAG ...]  ->  tools/bin/lib<FILE>_<NAME>.so: the whole library built with the
# flags by the Makefile's variant recipe, objects in tools/bin/obj_<FILE>_<NAME> (the switches the trace kernels know: artist_amd/csrc/trace_diag.hpp;
# SRC = an edited copy of <FILE>.hip to compile in its place, e.g. one with a seeded arithmetic error to show that a test can fail: load the result
# with ARTIST_HIP_LIB)
set -e
here="$(cd "$(dirname "$0")" && pwd)"
[ -z "$SRC" ] || SRC="$(cd "$(dirname "$SRC")" && pwd)/$(basename "$SRC")"
file=$1; name=$2; shift; shift
make -C "$here/../artist_amd/csrc" -j16 DIAG="$* -I." OBJDIR=../../tools/bin/obj_${file}_$name OUT=../../tools/bin/lib${file}_$name.so ${SRC:+SRC_$file=$SRC}
