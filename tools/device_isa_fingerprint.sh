#!/bin/bash
# device_isa_fingerprint.sh <csrc dir> <out dir>: device-only gfx950 ISA of every k_*.hip translation unit, each with its object's own flags (`make isa` of
# this tree's csrc/Makefile, run on the given csrc directory - which may be another checkout's), and one hash per unit: for bitwise comparisons of refactors
# (tools/isa_identity.py compares two such directories kernel by kernel)
set -e
src=$(cd "$1" && pwd); mkdir -p "$2"; out=$(cd "$2" && pwd)
make -s -C "$src" -f "$(cd "$(dirname "$0")/../amuse_amd/csrc" && pwd)/Makefile" -j8 isa OUT="$out" 2>/dev/null
cd "$out" && for f in *.s; do grep -v "^\s*\.\(file\|ident\|section\|loc\)\|^\s*;" $f | sed 's/\s*;.*$//' | sha256sum | cut -c1-16 | tr '\n' ' '; echo $f; done
