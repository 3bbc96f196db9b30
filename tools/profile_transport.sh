#!/bin/bash
# Tendencies::computeTransportTendencies at QU30 size (tools/probes/transport_diag.py): device-event timing of the two
# group calls (twice: their own spread), of the fused transport call, of one Split-Explicit step with the fused transport
# off and on, and of one fused RHS in the same process (no profiler), bounded by timeout.
# A run that fails or times out ends the script with its log tail and a non-zero exit: no further GPU step after it.
#   usage: [OUT_DIR=dir] bash tools/profile_transport.sh <tag> [transport_diag.py args]
#   -> $OUT_DIR/<tag>_*   (OUT_DIR defaults to build/profile_out, which git ignores)
NAME=transport LOG=transport_
. "$(dirname "$0")/profile_lib.sh"
step diag 500 python3 tools/probes/transport_diag.py "$@" --out $OUT/${TAG}_transport_diag_qu30.json
cat $OUT/${TAG}_transport_diag_qu30.json
