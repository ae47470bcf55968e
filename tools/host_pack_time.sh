#!/bin/bash
# host_pack_time.sh OLD_TREE NEW_TREE [reps]: ms of amuse_update_weights(AMUSE_UPD_ALL) on the stubbed runtime, -O3 without sanitizers, the two trees in alternation
# (one process per repetition: context creation is the warm-up of its update); prints both series with median and spread
set -e
old=$1; new=$2; reps=${3:-7}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
here="$(cd "$(dirname "$0")" && pwd)"
tmp=$(mktemp -d)
for side in old new; do
  tree=${!side}; mkdir -p $tmp/$side
  for f in amuse_api amuse_variants amuse_audio_api; do
    $HIPCC --offload-host-only -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -c "$tree/amuse_amd/csrc/$f.hip" -o $tmp/$side/$f.o
  done
  $HIPCC --offload-host-only -O3 -std=c++17 -x hip -c "$tree/tests/host_asan/hip_stub.cpp" -o $tmp/$side/hip_stub.o
  /opt/rocm/lib/llvm/bin/clang++ -O3 -std=c++17 -I"$tree/include" -c "$here/host_pack_time.cpp" -o $tmp/$side/main.o
  /opt/rocm/lib/llvm/bin/clang++ $tmp/$side/*.o -o $tmp/$side/pack_time
done
$tmp/old/pack_time > /dev/null; $tmp/new/pack_time > /dev/null   # warm-up
for i in $(seq $reps); do
  echo "old $($tmp/old/pack_time)"; echo "new $($tmp/new/pack_time)"
done | tee $tmp/series.txt
for side in old new; do
  grep "^$side" $tmp/series.txt | cut -d' ' -f2 | sort -n | awk -v s=$side '{v[NR]=$1} END {printf "%s: median %.1f ms, min %.1f, max %.1f, spread %.1f (n = %d)\n", s, (NR%2 ? v[(NR+1)/2] : (v[NR/2]+v[NR/2+1])/2), v[1], v[NR], v[NR]-v[1], NR}'
done
rm -r $tmp
