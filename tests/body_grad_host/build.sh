#!/bin/bash
# builds tests/body_grad_host/body_grad_host (the host code of amuse_body.hip + amuse_body_grad.hip, amuse_body_pack.hpp and the stubbed runtime of tests/host_asan,
# -fsanitize=address,undefined): build.sh <out dir>
set -e
here="$(cd "$(dirname "$0")" && pwd)"
out=${1:-/tmp/amuse_body_grad_host}
mkdir -p "$out"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1"
$HIPCC --offload-host-only -std=c++17 $SAN -Wno-unused-function -c "$here/../../amuse_amd/csrc/amuse_body.hip" -o "$out/amuse_body.o"
$HIPCC --offload-host-only -std=c++17 $SAN -Wno-unused-function -c "$here/../../amuse_amd/csrc/amuse_body_grad.hip" -o "$out/amuse_body_grad.o"
$HIPCC --offload-host-only -std=c++17 $SAN -x hip -c "$here/../host_asan/hip_stub.cpp" -o "$out/hip_stub.o"
$HIPCC --offload-host-only -std=c++17 $SAN -x hip -c "$here/main.cpp" -o "$out/main.o"
/opt/rocm/lib/llvm/bin/clang++ $SAN "$out/main.o" "$out/hip_stub.o" "$out/amuse_body.o" "$out/amuse_body_grad.o" -o "$out/body_grad_host"
