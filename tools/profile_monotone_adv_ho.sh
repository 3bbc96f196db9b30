#!/bin/bash
# The high-order horizontal flux of MonotoneAdv at QU30 size (tools/probes/monotone_adv_ho_diag.py): device-event timing
# of addTracerTend at orders 2 (the centred form: the yardstick, same binary, same run), 3 and 4, and of one attached
# Split-Explicit step at each, each twice in the same process (no profiler); then rocprofv3 --kernel-trace --stats of
# addTracerTend alone at orders 2 and 4, which splits each call into its launches.  Every step is bounded by timeout.
# A run that fails or times out ends the script with its log tail and a non-zero exit: no further GPU step after it.
#   usage: [OUT_DIR=dir] bash tools/profile_monotone_adv_ho.sh <tag> [monotone_adv_ho_diag.py args]
#   -> $OUT_DIR/<tag>_*   (OUT_DIR defaults to build/profile_out, which git ignores)
set -o pipefail
TAG=${1:?tag}; shift
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${OUT_DIR:-build/profile_out}
mkdir -p $OUT
timeout -k 10 540 python3 tools/probes/monotone_adv_ho_diag.py "$@" --out $OUT/${TAG}_monotone_adv_ho_diag_qu30.json > $OUT/${TAG}_monotone_adv_ho_diag.log 2>&1
rc=$?
echo "[monotone_adv_ho] diag rc=$rc"
if [ $rc -ne 0 ]; then
   echo "[monotone_adv_ho] diag FAILED (rc $rc; 124 = timeout): last lines of its log" >&2
   tail -20 $OUT/${TAG}_monotone_adv_ho_diag.log >&2
   exit $rc
fi
cat $OUT/${TAG}_monotone_adv_ho_diag_qu30.json
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_monotone_adv_ho_trace -o t -- \
   python3 tools/probes/monotone_adv_ho_diag.py "$@" --only-kernels --iters 20 > $OUT/${TAG}_monotone_adv_ho_trace.log 2>&1
rc=$?
echo "[monotone_adv_ho] trace rc=$rc"
if [ $rc -ne 0 ]; then
   echo "[monotone_adv_ho] trace FAILED (rc $rc; 124 = timeout): last lines of its log" >&2
   tail -20 $OUT/${TAG}_monotone_adv_ho_trace.log >&2
   exit $rc
fi
# the tile kernels' mean durations go into the record as "kernel_trace_ms"
python3 - $OUT/${TAG}_monotone_adv_ho_trace $OUT/${TAG}_monotone_adv_ho_diag_qu30.json <<'PY'
import csv, glob, json, re, sys
rows = {}
for f in glob.glob(sys.argv[1] + "/**/*kernel_stats.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        m = re.search(r"(Mono\w+Body\w*(?:<[\w, ]+>)?)", r["Name"])
        if m:
            rows[m.group(1)] = {"calls": int(r["Calls"]), "mean_ms": float(r["AverageNs"]) / 1.0e6}
rec = json.load(open(sys.argv[2]))
rec["kernel_trace_ms"] = rows
open(sys.argv[2], "w").write(json.dumps(rec) + "\n")
print(json.dumps(rows))
PY
exit $?
