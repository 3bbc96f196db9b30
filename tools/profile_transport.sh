#!/bin/bash
# Tendencies::computeTransportTendencies at QU30 size (tools/probes/transport_diag.py): device-event timing of the two
# group calls (twice: their own spread), of the fused transport call, of one Split-Explicit step with the fused transport
# off and on, and of one fused RHS in the same process (no profiler), bounded by timeout.
# A run that fails or times out ends the script with its log tail and a non-zero exit: no further GPU step after it.
#   usage: [OUT_DIR=dir] bash tools/profile_transport.sh <tag> [transport_diag.py args]
#   -> $OUT_DIR/<tag>_*   (OUT_DIR defaults to build/profile_out, which git ignores)
set -o pipefail
TAG=${1:?tag}; shift
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${OUT_DIR:-build/profile_out}
mkdir -p $OUT
timeout -k 10 500 python3 tools/probes/transport_diag.py "$@" --out $OUT/${TAG}_transport_diag_qu30.json > $OUT/${TAG}_transport_diag.log 2>&1
rc=$?
echo "[transport] diag rc=$rc"
if [ $rc -ne 0 ]; then
   echo "[transport] diag FAILED (rc $rc; 124 = timeout): last lines of its log" >&2
   tail -20 $OUT/${TAG}_transport_diag.log >&2
   exit $rc
fi
cat $OUT/${TAG}_transport_diag_qu30.json
exit 0
