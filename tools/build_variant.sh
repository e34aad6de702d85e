#!/bin/bash
# Build an A/B variant of libcnngp into cnn-gp_amd/lib/ab/lib_<name>.so (tools/gpu.sh ab /
# tools/ab_variant.sh time it; CNNGP_LIB selects it).  The variant has every entry point: the
# object list is the Makefile's.
#   bash tools/build_variant.sh NAME "-DFOO=1 -DBAR=0"
#       netfuse.hip (default), cnngp.hip (VARIANT_SRC=cnngp) or both (VARIANT_SRC=both)
#       compiled with the extra flags, linked with the regular objects of the rest
#   VARIANT_TREE=DIR bash tools/build_variant.sh NAME
#       the library of another checkout as it stands, e.g. a `git worktree` of the parent
#       commit, built by that checkout's own Makefile
set -eu
cd "$(dirname "$0")/../cnn-gp_amd/csrc"
NAME=$1; DEFS=${2:-}; SRC=${VARIANT_SRC:-netfuse}
ROCM=/opt/rocm
mkdir -p build/ab ../lib/ab
if [ -n "${VARIANT_TREE:-}" ]; then
    make -s -C "$VARIANT_TREE/cnn-gp_amd/csrc" -j"${JOBS:-8}"
    cp "$VARIANT_TREE/cnn-gp_amd/lib/libcnngp.so" "../lib/ab/lib_$NAME.so"
    echo "built lib/ab/lib_$NAME.so (tree $VARIANT_TREE)"
    exit 0
fi
FL="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Wall -I../../include -I$ROCM/include"
OBJS=$(make -s --eval='print-objs: ; @echo $(OBJS)' print-objs)
make -s -j"${JOBS:-8}" $OBJS
LINK=""
for o in $OBJS; do
    u=$(basename "$o" .o)
    if [ "$u" = "$SRC" ] || { [ "$SRC" = both ] && { [ "$u" = cnngp ] || [ "$u" = netfuse ]; }; }; then
        $ROCM/bin/hipcc $FL $DEFS -c "$u.hip" -o "build/ab/${u}_$NAME.o"
        o="build/ab/${u}_$NAME.o"
    fi
    LINK="$LINK $o"
done
$ROCM/bin/hipcc $FL $LINK -shared -L$ROCM/lib -lrocsolver -lrocblas -Wl,-rpath,$ROCM/lib -o ../lib/ab/lib_$NAME.so
echo "built lib/ab/lib_$NAME.so ($SRC $DEFS)"
