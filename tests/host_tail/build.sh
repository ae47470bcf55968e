#!/bin/bash
# builds tests/host_tail/{host_tail,host_notail} (the host code of the audio model's tail + stubbed runtime, -fsanitize=address,undefined): build.sh <out dir>
# host_tail links amuse_audio_tail.o and the stubs of its launchers; host_notail links what tests/host_asan/build.sh links and nothing else.
set -e
here="$(cd "$(dirname "$0")" && pwd)"
out=${1:-/tmp/amuse_host_tail}
mkdir -p "$out"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
CXX=/opt/rocm/lib/llvm/bin/clang++
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1"
for f in amuse_api amuse_variants amuse_audio_api amuse_audio_tail; do
  $HIPCC --offload-host-only -std=c++17 $SAN -Wno-unused-function -c "$here/../../amuse_amd/csrc/$f.hip" -o "$out/$f.o"
done
$HIPCC --offload-host-only -std=c++17 $SAN -x hip -c "$here/../host_asan/hip_stub.cpp" -o "$out/hip_stub.o"
$HIPCC --offload-host-only -std=c++17 $SAN -x hip -c "$here/tail_stub.cpp" -o "$out/tail_stub.o"
$CXX -std=c++17 $SAN -c "$here/main.cpp" -o "$out/main.o"
$CXX $SAN "$out/main.o" "$out/hip_stub.o" "$out/tail_stub.o" "$out/amuse_api.o" "$out/amuse_variants.o" "$out/amuse_audio_api.o" "$out/amuse_audio_tail.o" -o "$out/host_tail"
$CXX $SAN "$out/main.o" "$out/hip_stub.o" "$out/amuse_api.o" "$out/amuse_variants.o" "$out/amuse_audio_api.o" -o "$out/host_notail"
