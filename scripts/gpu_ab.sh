#!/bin/bash
# A/B of two library builds on the same box, interleaved: scripts/gpu_ab.sh "<extra hipcc flags for B>" [bench args]
FLAGS="$1"; shift
python -m opticalflow_amd.build --force --output opticalflow_amd/csrc/libvof_b.so -- $FLAGS
for i in 1 2; do
  echo "--- A (default build)"; python bench.py --full --steps 2 --no-cpu-baseline --profile-table "$@" 2>&1 | grep -E "^  (gs|apply0|residual) .*L[01] |value" | cut -c1-118
  echo "--- B ($FLAGS)"; VOF_LIB=$PWD/opticalflow_amd/csrc/libvof_b.so python bench.py --full --steps 2 --no-cpu-baseline --profile-table "$@" 2>&1 | grep -E "^  (gs|apply0|residual) .*L[01] |value" | cut -c1-118
done
