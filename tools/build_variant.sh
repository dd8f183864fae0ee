#!/bin/bash
# A/B builds of the particle kernels with other compile-time constants (development tool):
#   tools/build_variant.sh NAME FILE "-DFY_FORCE_LOG2=10 ..."   ->  yade-openfoam-coupling_amd/lib/variants/libfoamyade_hip_NAME.so
# select at run time with FOAMYADE_HIP_LIB=<that path>.  Only FILE (a source of csrc/) is recompiled; the other objects are the default build's.
# Which constant lives in which file:
#   particle_force.hip    FY_FORCE_THREADS, FY_FORCE_LOG2, FY_FORCE_ATTR
#   particle_locate.hip   FY_DEP_THREADS, FY_DEP_LOG2, FY_DEP_ATTR, FY_LD_ATTR, FY_LOC_REFILL
# VARIANT_REPLACES=<source of the Makefile's list>: FILE is another file (an older revision, a timing-only copy) that stands in for that source.
set -e
cd "$(dirname "$0")/../yade-openfoam-coupling_amd/csrc"
if [ $# -lt 2 ] || [ ! -f "$2" ]; then echo "usage: $0 NAME FILE [compiler flags ...]   (FILE: a source in $(pwd))" >&2; exit 2; fi
name=$1; src=$2; shift 2
make -s all
mkdir -p ../build/variants ../lib/variants
repl=${VARIANT_REPLACES:-$src}      # the default object the variant stands in for
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -munsafe-fp-atomics -Wall -Wno-unused-result "$@" -x hip -c $src -o ../build/variants/${src}_$name.o
objs=""; found=0
for f in $(make -s print-src); do      # the Makefile's SRC: one list of the library's sources
  if [ "$f" == "$repl" ]; then objs="$objs ../build/variants/${src}_$name.o"; found=1; else objs="$objs ../build/$f.o"; fi
done
if [ $found == 0 ]; then echo "$repl is not one of the library's sources" >&2; exit 2; fi
hipcc --offload-arch=gfx950 -shared -fPIC -o ../lib/variants/libfoamyade_hip_$name.so $objs -pthread -ldl
echo built ../lib/variants/libfoamyade_hip_$name.so
