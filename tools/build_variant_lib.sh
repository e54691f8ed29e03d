#!/bin/bash
# Builds raytracing-book_amd/lib/<tag>/librtamd.so from the working tree's kernel source with extra
# compiler definitions (ablations and A/B forms, e.g. -DRT_ABL_UNITVEC1) and the working tree's
# C ABI object, for tools/lib_ab.py.  usage: tools/build_variant_lib.sh <tag> <-Dflags...>
# The scene-8 kernels' other forms (rt_kernel_common.h): -DRT_WT_DISPATCH=0 the leaf stage's record
# address by a branch cascade, -DRT_WT_FIRST_LEAF=0 without the first-leaf prologue, -DRT_PB_NOLIGHT=0 the
# mixture of shade() as every other kernel has it.
set -e
TAG=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
PKG=$ROOT/raytracing-book_amd
TMP=$(mktemp -d)
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -fPIC -Wno-unused-variable -Wno-unused-function"
INC="-I$ROOT/include -I$PKG/csrc -I$PKG/host"
/opt/rocm/bin/hipcc $FLAGS $INC "$@" -c -o "$TMP/k.o" "$PKG/csrc/rt_kernel.hip"
mkdir -p "$PKG/lib/$TAG"
# the working tree's C-ABI objects: the Makefile holds the list (make builds them)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$PKG/lib/$TAG/librtamd.so" "$TMP/k.o" $(make -s -C "$PKG" print-abi-objs)
rm -rf "$TMP"
echo "built $PKG/lib/$TAG/librtamd.so with $*"
