#!/bin/bash
# Tendencies::computeMomentumTendencies and computeTransportTendenciesAndUpdate at QU30 size
# (tools/probes/momentum_update_diag.py): device-event timing of one fused RHS, of the momentum-only RHS, of the transport
# call with the two update kernels (twice: their own spread), of the folded call with the tendencies kept and dropped, and
# of one Split-Explicit step under each combination of the two switches, in the same process (no profiler), bounded by
# timeout.  A run that fails or times out ends the script with its log tail and a non-zero exit: no further GPU step
# after it.
#   usage: [OUT_DIR=dir] bash tools/profile_momentum_update.sh <tag> [momentum_update_diag.py args]
#   -> $OUT_DIR/<tag>_*   (OUT_DIR defaults to build/profile_out, which git ignores)
NAME=momentum_update LOG=momentum_update_
. "$(dirname "$0")/profile_lib.sh"
step diag 540 python3 tools/probes/momentum_update_diag.py "$@" --out $OUT/${TAG}_momentum_update_diag_qu30.json
cat $OUT/${TAG}_momentum_update_diag_qu30.json
