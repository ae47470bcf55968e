#!/bin/bash
# builds tests/bvh_host/bvh_host (amuse_bvh.hip's host code + amuse_bvh_host.hpp on stand-in launchers, -fsanitize=address,undefined): build.sh <out dir>
set -e
here="$(cd "$(dirname "$0")" && pwd)"
out=${1:-/tmp/amuse_bvh_host}
mkdir -p "$out"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1"
$HIPCC --offload-host-only -std=c++17 $SAN -Wno-unused-function -c "$here/../../amuse_amd/csrc/amuse_bvh.hip" -o "$out/amuse_bvh.o"
$HIPCC --offload-host-only -std=c++17 $SAN -x hip -c "$here/../host_asan/hip_stub.cpp" -o "$out/hip_stub.o"
$HIPCC --offload-host-only -std=c++17 $SAN -x hip -c "$here/main.cpp" -o "$out/main.o"
/opt/rocm/lib/llvm/bin/clang++ $SAN "$out/main.o" "$out/hip_stub.o" "$out/amuse_bvh.o" -o "$out/bvh_host"
