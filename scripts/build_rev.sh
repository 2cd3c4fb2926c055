#!/bin/bash
# Builds the product library of a git revision for a same-box A/B (scripts/ab.py):
#   scripts/build_rev.sh <git-rev> <tag>   ->  smcdet_amd/libsmcdet_hip_<tag>.so
# The revision's tree is exported (git archive, local) to build/rev_<tag>/ and
# built there with its own Makefile, so the object list is that revision's.
# A host-side step: run it where the sources are compiled, not on the GPU box.
set -euo pipefail
cd "$(dirname "$0")/.."
if [ $# -ne 2 ]; then echo "usage: $0 <git-rev> <tag>" >&2; exit 2; fi
rev=$(git rev-parse --verify "$1^{commit}"); tag=$2
D=build/rev_$tag
rm -rf "$D"
mkdir -p "$D"
git archive "$rev" | tar -x -C "$D"
make -C "$D" -j"${JOBS:-16}" smcdet_amd/libsmcdet_hip.so
cp "$D/smcdet_amd/libsmcdet_hip.so" "smcdet_amd/libsmcdet_hip_$tag.so"
echo "built smcdet_amd/libsmcdet_hip_$tag.so from $rev"
