#!/bin/bash
# Build libnaima_hip.so for gfx950 (MI355X) in-tree.  hipcc cross-compiles
# without a GPU.  Usage: naima_amd/csrc/build.sh [extra hipcc flags]
set -euo pipefail
here="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
out="${NH_OUT:-$here/../libnaima_hip.so}"
tmp="$out.tmp.$$"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
"$HIPCC" --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared \
  -Wall -Wno-unused-function -mllvm -amdgpu-kernarg-preload-count=16 "$@" \
  "$here/nh_core.hip" "$here/nh_synchrotron.hip" "$here/nh_tables.hip" "$here/nh_device.hip" "$here/nh_moves.hip" "$here/nh_comm.hip" "$here/nh_kelner.hip" "$here/nh_kelner_leptons.hip" "$here/nh_halfstep.hip" "$here/nh_persist.hip" "$here/nh_general.hip" "$here/nh_select.hip" "$here/nh_autocorr.hip" "$here/nh_ebl.hip" "$here/nh_pairabs.hip" "$here/nh_ssa.hip" "$here/nh_cooling.hip" "$here/nh_thin.hip" "$here/nh_posterior.hip" "$here/nh_infocrit.hip" "$here/nh_rank.hip" "$here/nh_predictive.hip" "$here/nh_evidence.hip" "$here/nh_reweight.hip" "$here/nh_simplex.hip" \
  -ldl -lpthread -o "$tmp"
mv -f "$tmp" "$out"  # (atomic: a snapshot of the tree never sees a half-written library)
echo "built $out"
