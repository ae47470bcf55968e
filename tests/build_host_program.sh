#!/bin/bash
# builds the stand-alone host program tests/<unit>_host/main.cpp as <out dir>/<unit>_host: the host code of csrc/amuse_<unit>.hip (and of any further csrc units
# named) on stand-in launchers and the stubbed runtime of tests/host_asan, -fsanitize=address,undefined: build_host_program.sh <unit> <out dir> [csrc units...]
set -e
here="$(cd "$(dirname "$0")" && pwd)"
unit=$1
out=${2:-/tmp/amuse_${unit}_host}
mkdir -p "$out"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1"
objs=""
for f in "${@:3}" "amuse_$unit"; do
  $HIPCC --offload-host-only -std=c++17 $SAN -Wno-unused-function -c "$here/../amuse_amd/csrc/$f.hip" -o "$out/$f.o"
  objs="$objs $out/$f.o"
done
$HIPCC --offload-host-only -std=c++17 $SAN -x hip -c "$here/host_asan/hip_stub.cpp" -o "$out/hip_stub.o"
$HIPCC --offload-host-only -std=c++17 $SAN -x hip -c "$here/${unit}_host/main.cpp" -o "$out/main.o"
/opt/rocm/lib/llvm/bin/clang++ $SAN "$out/main.o" "$out/hip_stub.o" $objs -o "$out/${unit}_host"
