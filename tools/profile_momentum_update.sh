#!/bin/bash
# Tendencies::computeMomentumTendencies and computeTransportTendenciesAndUpdate at QU30 size
# (tools/probes/momentum_update_diag.py): device-event timing of one fused RHS, of the momentum-only RHS, of the transport
# call with the two update kernels (twice: their own spread), of the folded call with the tendencies kept and dropped, and
# of one Split-Explicit step under each combination of the two switches, in the same process (no profiler), bounded by
# timeout.  A run that fails or times out ends the script with its log tail and a non-zero exit: no further GPU step
# after it.
#   usage: [OUT_DIR=dir] bash tools/profile_momentum_update.sh <tag> [momentum_update_diag.py args]
#   -> $OUT_DIR/<tag>_*   (OUT_DIR defaults to build/profile_out, which git ignores)
set -o pipefail
TAG=${1:?tag}; shift
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${OUT_DIR:-build/profile_out}
mkdir -p $OUT
timeout -k 10 540 python3 tools/probes/momentum_update_diag.py "$@" --out $OUT/${TAG}_momentum_update_diag_qu30.json > $OUT/${TAG}_momentum_update_diag.log 2>&1
rc=$?
echo "[momentum_update] diag rc=$rc"
if [ $rc -ne 0 ]; then
   echo "[momentum_update] diag FAILED (rc $rc; 124 = timeout): last lines of its log" >&2
   tail -20 $OUT/${TAG}_momentum_update_diag.log >&2
   exit $rc
fi
cat $OUT/${TAG}_momentum_update_diag_qu30.json
exit 0
