#!/bin/bash
# The int8 stage alone on several builds of the library, same box, in the order given: gpu_i8_attribution.sh label=lib.so label=lib.so ...
# (libraries relative to tensorrec_amd/; the stamped ones come from `make -C tensorrec_amd/csrc diag`, a build of the parent's kernel
# from a checkout of the parent's score_blockmax_i8.hip).  Every run has its own time limit and the first failure ends the script.
#   -> <out>/i8_stage_attribution_<label>.json each, merged into <out>/i8_stage_attribution.json (kept as profiles/i8_stage_attribution.json);
#   <out>: $TREC_OUT_DIR, bench_outputs/ in the repository root without it
set -o pipefail
cd "$(dirname "$0")/.."; export TREC_OUT_DIR="${TREC_OUT_DIR:-$PWD/bench_outputs}"; mkdir -p "$TREC_OUT_DIR"
LABELS=""
for A in "$@"; do
  LB="${A%%=*}"; LIB="${A#*=}"
  TREC_HIP_LIB=$PWD/tensorrec_amd/$LIB timeout -k 10 150 python scripts/i8_stage_attribution.py "$LB" 3 2>&1 | tail -3 || exit 1
  LABELS="$LABELS $LB"
done
python scripts/i8_stage_attribution.py --merge $LABELS
