#!/bin/bash
# Fast variant build: recompile only kernels/ptgsk.hip with extra flags and link it with the
# regular objects in shyft_amd/csrc/_obj (run `make -C shyft_amd/csrc` first).
# usage: build_variants_ptgsk.sh name1 "flags1" name2 "flags2" ...
# e.g. the Brent opening A/B:
#   build_variants_ptgsk.sh bopen0 "-DSHYFT_PTGSK_BOPEN=0" bopen1 "-DSHYFT_PTGSK_BOPEN=1" bopen2 "-DSHYFT_PTGSK_BOPEN=2"
# or the incomplete gamma's term loops (device/gamma_lean.h): gl0 "-DSHYFT_GAMMA_LOOPS=0" gl3 "-DSHYFT_GAMMA_LOOPS=3"
# PTGSK_FLAGS: the Makefile's per-object flags of this file (set it empty to build a variant without them)
set -e
cd "$(dirname "$0")/../shyft_amd/csrc"
OUTD=${OUT:-tools/variants}; mkdir -p ../../$OUTD
PTGSK_FLAGS=${PTGSK_FLAGS--mllvm -disable-machine-licm}
others=$(ls _obj/*.o _obj/kernels/*.o | grep -v "kernels/ptgsk.o")
while [ $# -gt 1 ]; do
  name=$1; flags=$2; shift 2
  (/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off $PTGSK_FLAGS $flags -c kernels/ptgsk.hip -o /tmp/ptgsk_$name.o &&
   /opt/rocm/bin/hipcc -O3 -fPIC --offload-arch=gfx950 -shared -o ../../$OUTD/$name.so $others /tmp/ptgsk_$name.o -lrocblas -lrccl &&
   echo built $name) &
done
wait
