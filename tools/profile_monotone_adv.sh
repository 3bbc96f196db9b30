#!/bin/bash
# MonotoneAdv at QU30 size (tools/probes/monotone_adv_diag.py): device-event timing of the transport call with the built-in
# centred advection, of the same call without it followed by MonotoneAdv::addTracerTend, of addTracerTend alone, and of one
# Split-Explicit step without and with the attachment, each twice in the same process (no profiler), bounded by timeout.
# A run that fails or times out ends the script with its log tail and a non-zero exit: no further GPU step after it.
#   usage: [OUT_DIR=dir] bash tools/profile_monotone_adv.sh <tag> [monotone_adv_diag.py args]
#   -> $OUT_DIR/<tag>_*   (OUT_DIR defaults to build/profile_out, which git ignores)
set -o pipefail
TAG=${1:?tag}; shift
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${OUT_DIR:-build/profile_out}
mkdir -p $OUT
timeout -k 10 500 python3 tools/probes/monotone_adv_diag.py "$@" --out $OUT/${TAG}_monotone_adv_diag_qu30.json > $OUT/${TAG}_monotone_adv_diag.log 2>&1
rc=$?
echo "[monotone_adv] diag rc=$rc"
if [ $rc -ne 0 ]; then
   echo "[monotone_adv] diag FAILED (rc $rc; 124 = timeout): last lines of its log" >&2
   tail -20 $OUT/${TAG}_monotone_adv_diag.log >&2
   exit $rc
fi
cat $OUT/${TAG}_monotone_adv_diag_qu30.json
exit 0
