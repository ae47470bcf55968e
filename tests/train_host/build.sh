#!/bin/bash
# builds tests/train_host/train_host (the training step's translation units as they are, host side only, on the stubbed runtime of tests/host_asan at its raw launch
# level, -fsanitize=address,undefined): build.sh <out dir>.  CSRC=<dir> builds another tree's amuse_amd/csrc with this driver and stub (how the golden was recorded).
set -e
here="$(cd "$(dirname "$0")" && pwd)"
out=${1:-/tmp/amuse_train_host}
csrc=${CSRC:-$here/../../amuse_amd/csrc}
mkdir -p "$out"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1"
objs=""
for f in amuse_train k_train k_train_attn k_train_gemm; do
  [ -f "$csrc/$f.hip" ] || continue   # (amuse_train.hip: not in the tree the golden was recorded from)
  $HIPCC --offload-host-only -std=c++17 $SAN -Wno-unused-function -c "$csrc/$f.hip" -o "$out/$f.o"
  objs="$objs $out/$f.o"
done
$HIPCC --offload-host-only -std=c++17 $SAN -x hip -c "$here/../host_asan/hip_stub.cpp" -o "$out/hip_stub.o"
/opt/rocm/lib/llvm/bin/clang++ -std=c++17 $SAN -c "$here/main.cpp" -o "$out/main.o"
# (the kernels' host stubs refer to the device image's data symbols, which a host-only build does not have and nothing here reads)
/opt/rocm/lib/llvm/bin/clang++ $SAN -Wl,--unresolved-symbols=ignore-all "$out/main.o" "$out/hip_stub.o" $objs -o "$out/train_host"
