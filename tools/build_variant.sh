#!/bin/bash
# build libamuse_hip variants with extra -D flags for A/B timing: tools/build_variant.sh NAME SOURCE.hip "-DX=1 ..."
# (SOURCE = the one translation unit that is recompiled, e.g. k_sampler8.hip or k_vae_fused.hip; the other objects - the Makefile's
# list, `make -s print-obj` - are taken from the regular build, which must be up to date)
set -e
cd "$(dirname "$0")/../amuse_amd/csrc"
name=$1; src=$2; shift 2
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function $@ -c $src -o /tmp/${src%.hip}_$name.o
objs=""
for o in $(make -s print-obj); do
  if [ "${o%.o}.hip" == "$src" ]; then objs="$objs /tmp/${o%.o}_$name.o"; else objs="$objs $o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libamuse_hip_$name.so $objs
