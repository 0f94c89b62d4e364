#!/bin/bash
# Device assembly of translation units, for before/after comparisons of a refactoring that must
# not change the generated code:  tools/isa_dump.sh <outdir> [unit ...]
# Without units: the free-gas ones, ndpp_hip (product arithmetic, -> fast.s) and fg_strict_stages
# (-> strict.s).  A unit is a file of ndpp_amd/csrc without its .hip (file6_kernels, tab_kernels, ...),
# compiled the way the always-strict units are.
# (then: diff a/<unit>.code b/<unit>.code -- the __hip_cuid_ symbol differs between any two builds;
# block labels lose their function number, so that removing one kernel does not renumber the rest)
set -e
out=${1:?outdir}; mkdir -p "$out"; shift
src=$(dirname "$0")/../ndpp_amd/csrc
strict="-DNDPP_FAST=0 -ffp-contract=off"
if [ $# -eq 0 ]; then
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -DNDPP_FAST=1 -ffp-contract=fast -S --cuda-device-only "$src/ndpp_hip.hip" -o "$out/fast.s" &
  hipcc --offload-arch=gfx950 -O3 -std=c++17 $strict -S --cuda-device-only "$src/fg_strict_stages.hip" -o "$out/strict.s" &
  set -- fast strict
else
  for u in "$@"; do
    hipcc --offload-arch=gfx950 -O3 -std=c++17 $strict -S --cuda-device-only "$src/$u.hip" -o "$out/$u.s" &
  done
fi
wait
for f in "$@"; do grep -v '^\s*[;.]' "$out/$f.s" | sed -E 's/;.*$//; s/LBB[0-9]+_/LBB_/g; s/Lfunc_(begin|end)[0-9]+/Lfunc_\1/g' > "$out/$f.code"; wc -l "$out/$f.code"; done
