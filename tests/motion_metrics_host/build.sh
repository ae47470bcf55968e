#!/bin/bash
# builds tests/motion_metrics_host/motion_metrics_host (amuse_motion_metrics.hip's host code + amuse_motion_metrics_host.hpp on a stand-in launcher,
# -fsanitize=address,undefined): build.sh <out dir>
set -e
here="$(cd "$(dirname "$0")" && pwd)"
out=${1:-/tmp/amuse_motion_metrics_host}
mkdir -p "$out"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1"
$HIPCC --offload-host-only -std=c++17 $SAN -Wno-unused-function -c "$here/../../amuse_amd/csrc/amuse_motion_metrics.hip" -o "$out/amuse_motion_metrics.o"
$HIPCC --offload-host-only -std=c++17 $SAN -x hip -c "$here/../host_asan/hip_stub.cpp" -o "$out/hip_stub.o"
$HIPCC --offload-host-only -std=c++17 $SAN -x hip -c "$here/main.cpp" -o "$out/main.o"
/opt/rocm/lib/llvm/bin/clang++ $SAN "$out/main.o" "$out/hip_stub.o" "$out/amuse_motion_metrics.o" -o "$out/motion_metrics_host"
