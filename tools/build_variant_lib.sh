#!/bin/bash
# Builds raytracing-book_amd/lib/<tag>/librtamd.so from the working tree's kernel source with extra
# compiler definitions (ablations and A/B forms, e.g. -DRT_ABL_UNITVEC1) and the working tree's
# C ABI object, for tools/lib_ab.py.  usage: tools/build_variant_lib.sh <tag> <-Dflags...>
# The kernels' compile-time A/B switches (RT_BL_SPAIR, RT_BL_STEPS, RT_WT_DISPATCH, RT_WT_FIRST_LEAF,
# RT_PB_NOLIGHT) are one block at the top of raytracing-book_amd/csrc/rt_kernel_common.h, each with
# what its other form builds: e.g. -DRT_WT_FIRST_LEAF=0.
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
