#!/bin/bash
# MonotoneAdv at QU30 size (tools/probes/monotone_adv_diag.py --form 2d|3d|ho, which lists the cases of each form):
# device-event timing of addTracerTend against the path the form replaces and of one Split-Explicit step each way, each
# twice in the same process (no profiler).  For the forms 3d and ho then, as a step of its own, rocprofv3 --kernel-trace
# --stats of addTracerTend alone (--only-kernels), which splits each call into its launches.  Every step is bounded by
# timeout.  A run that fails or times out ends the script with its log tail and a non-zero exit: no further GPU step
# after it.
#   usage: [OUT_DIR=dir] bash tools/profile_monotone_adv.sh <tag> [--form 2d|3d|ho] [monotone_adv_diag.py args]
#   -> $OUT_DIR/<tag>_*   (OUT_DIR defaults to build/profile_out, which git ignores)
FORM=2d
prev=
for arg in "${@:2}"; do
   [ "$prev" = --form ] && FORM=$arg
   case $arg in --form=*) FORM=${arg#--form=};; esac
   prev=$arg
done
case $FORM in
   2d) NAME=monotone_adv;;
   3d) NAME=monotone_adv3d;;
   ho) NAME=monotone_adv_ho;;
   *) echo "unknown form '$FORM'" >&2; exit 2;;
esac
LOG=${NAME}_
. "$(dirname "$0")/profile_lib.sh"
JSON=$OUT/${TAG}_${NAME}_diag_qu30.json
step diag 540 python3 tools/probes/monotone_adv_diag.py "$@" --out $JSON
cat $JSON
[ $FORM = 2d ] && exit 0
trace python3 tools/probes/monotone_adv_diag.py "$@" --only-kernels --iters 20
# the tile kernels' mean durations go into the record as "kernel_trace_ms"
python3 - $OUT/${TAG}_${NAME}_trace $JSON <<'PY'
import json, re, sys
sys.path.insert(0, ".")
from tools.summarise_profile import kernel_stats
rows = {}
for r in kernel_stats(sys.argv[1]):
    m = re.search(r"(Mono\w+Body\w*(?:<[\w, ]+>)?)", r["Name"])
    if m:
        rows[m.group(1)] = {"calls": int(r["Calls"]), "mean_ms": float(r["AverageNs"]) / 1.0e6}
rec = json.load(open(sys.argv[2]))
rec["kernel_trace_ms"] = rows
open(sys.argv[2], "w").write(json.dumps(rec) + "\n")
print(json.dumps(rows))
PY
exit $?
