#!/bin/bash
# build/variants/<name>.so: the library with extra compiler flags on vspg_capi.hip (every other object of the Makefile's OBJS is reused
# as built; WF=1 recompiles the wavefront pipeline's two with the flags as well), for same-box A/Bs through VSPG_LIB
# (scripts/gpu_variants.sh):  bash scripts/build_variant.sh <name> "<flags>"
set -e
NAME=$1; FLAGS=$2
cd "$(dirname "$0")/../vspg-pbrt-v4_amd/csrc"
HIPFLAGS=$(make -s --no-print-directory print-HIPFLAGS)
OBJS=$(make -s --no-print-directory print-OBJS)   # the flags and the object list are the Makefile's: nothing to keep in step here
OBJS=" $OBJS "; OBJS=${OBJS/ vspg_capi.o / }
OUT=../../build/variants; mkdir -p $OUT
/opt/rocm/bin/hipcc $HIPFLAGS $FLAGS -c -o $OUT/$NAME.capi.o vspg_capi.hip
if [ "${WF:-0}" = 1 ]; then
  /opt/rocm/bin/hipcc $HIPFLAGS $FLAGS -c -o $OUT/$NAME.wf_grid.o vspg_wf_grid.hip &
  /opt/rocm/bin/hipcc $HIPFLAGS $FLAGS -c -o $OUT/$NAME.wf_nvdb.o vspg_wf_nvdb.hip & wait
  OBJS=${OBJS/ vspg_wf_grid.o / $OUT/$NAME.wf_grid.o }; OBJS=${OBJS/ vspg_wf_nvdb.o / $OUT/$NAME.wf_nvdb.o }
fi
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fPIC -shared -o $OUT/$NAME.so $OUT/$NAME.capi.o $OBJS
echo built $OUT/$NAME.so
