#!/bin/bash
# Builds raytracing-book_amd/lib/prev/librtamd.so from a previous revision's kernel source, device
# headers and built-ins (default HEAD) and the working tree's C ABI, for tools/lib_ab.py.  The two kernels must
# share rt_device.h's argument layout.  usage: tools/build_prev_lib.sh [rev]
set -e
REV=${1:-HEAD}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
PKG=$ROOT/raytracing-book_amd
TMP=$(mktemp -d)
CSRC=raytracing-book_amd/csrc
git -C "$ROOT" show "$REV:$CSRC/rt_kernel.hip" > "$TMP/rt_kernel.hip"
# every header that revision has beside the kernel source (the shared device code, the launch code,
# the fold step, the plan): found there before the working tree's, so the old kernel never compiles
# against a newer header
for h in $(git -C "$ROOT" ls-tree --name-only "$REV" "$CSRC/" | grep '\.h$'); do
    git -C "$ROOT" show "$REV:$h" > "$TMP/$(basename "$h")"
done
# the built-in definitions (rt_glsl.h) of that revision too: searched before the working tree's
mkdir -p "$TMP/include/rt"
git -C "$ROOT" show "$REV:include/rt/rt_glsl.h" > "$TMP/include/rt/rt_glsl.h"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -fPIC -Wno-unused-variable -Wno-unused-function"
INC="-I$TMP/include -I$ROOT/include -I$PKG/csrc -I$PKG/host"
/opt/rocm/bin/hipcc $FLAGS $INC -c -o "$TMP/k.o" "$TMP/rt_kernel.hip"
mkdir -p "$PKG/lib/prev"
# the working tree's C-ABI objects: the Makefile holds the list (make builds them)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$PKG/lib/prev/librtamd.so" "$TMP/k.o" $(make -s -C "$PKG" print-abi-objs)
rm -rf "$TMP"
echo "built $PKG/lib/prev/librtamd.so from $REV"
