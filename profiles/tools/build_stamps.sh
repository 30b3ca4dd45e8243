#!/bin/bash
# Diagnostic build of libptnn with in-kernel cycle stamps (-DPTNN_STAMPS; NOSTAMPS=1: without them, e.g. for -DPTNN_ABLATE=k in $EXTRA), one shape only (default REG 4 -> 1; pass
# "task I O" for another, e.g. `build_stamps.sh 1 34 2`).  Never the product.
# EXTRA=-DPTNN_STAMPS_MH adds the two points inside the packed kernel's Metropolis-Hastings phase (they drain the LDS queue: ptnn_diag.hpp).
set -e
cd "$(dirname "$0")/../.."
T=${1:-0}; I=${2:-4}; O=${3:-1}
C=parallel-tempering-neural-net_amd/csrc
DEF=${NOSTAMPS:+-DPTNN_NO_STAMPS_BUILD}; [ -z "$NOSTAMPS" ] && DEF=-DPTNN_STAMPS
# the shape's fixed-width packed kernels (PTNN_PACK_FIXED / PTNN_PACKM_FIXED of ptnn_shapes.hpp): the same entries, each an object of its own
entries() { grep "^#define $1(X)" $C/ptnn_shapes.hpp | grep -o "X($T, *$I, *$O, *[0-9]*)" | tr -d ' ' | tr -d '\n'; }
FIXED=$(entries PTNN_PACK_FIXED); FIXEDM=$(entries PTNN_PACKM_FIXED)
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC $DEF $EXTRA -DPTNN_SHAPES(X)=X($T,$I,$O) -DPTNN_PACK_FIXED(X)=$FIXED -DPTNN_PACKM_FIXED(X)=$FIXEDM"
HOST=""
for U in ptnn ptnn_analysis ptnn_checkpoint ptnn_text; do
    /opt/rocm/bin/hipcc $F -c -o /tmp/ptnn_stamps_$U.o $C/$U.hip
    HOST="$HOST /tmp/ptnn_stamps_$U.o"
done
/opt/rocm/bin/hipcc $F -DPTNN_T=$T -DPTNN_I=$I -DPTNN_O=$O -DPTNN_SHAPE_SYMBOL=ptnn_shape_${T}_${I}_${O} -c -o /tmp/ptnn_stamps_shape.o $C/ptnn_shape.hip
# the shape's analysis kernels: ptnn_analysis.o refers to their table
/opt/rocm/bin/hipcc $F -DPTNN_T=$T -DPTNN_I=$I -DPTNN_O=$O -DPTNN_SHAPE_SYMBOL=ptnn_ashape_${T}_${I}_${O} -c -o /tmp/ptnn_stamps_ashape.o $C/ptnn_analysis_shape.hip
for KIND in pack packm; do
    [ $KIND = pack ] && { LIST=$FIXED; MULTI=; } || { LIST=$FIXEDM; MULTI=-DPTNN_HC_MULTI; }
    for HC in $(echo "$LIST" | grep -o ',[0-9]*)' | tr -d ',)'); do
        /opt/rocm/bin/hipcc $F -DPTNN_T=$T -DPTNN_I=$I -DPTNN_O=$O -DPTNN_HC=$HC $MULTI -DPTNN_SHAPE_SYMBOL=ptnn_${KIND}_fixed_${T}_${I}_${O}_${HC} -c -o /tmp/ptnn_stamps_${KIND}_fixed_$HC.o $C/ptnn_shape.hip
        HOST="$HOST /tmp/ptnn_stamps_${KIND}_fixed_$HC.o"
    done
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o profiles/tools/libptnn_stamps.so $HOST /tmp/ptnn_stamps_shape.o /tmp/ptnn_stamps_ashape.o
echo built profiles/tools/libptnn_stamps.so
