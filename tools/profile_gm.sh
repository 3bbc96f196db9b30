#!/bin/bash
# GentMcWilliams at QU30 size (tools/probes/gm_diag.py), four runs of their own, each bounded by timeout:
#   1. device-event timing of the bolus-velocity launch, the displaced column pass, step 5b and the yardsticks
#      (applyVelocityVertMix, one fused momentum RHS), alternating in one loop (no profiler)
#   2. rocprofv3 --kernel-trace --stats of the launch alone
#   3. rocprofv3 --pmc FETCH_SIZE, 4. rocprofv3 --pmc WRITE_SIZE TCC_HIT_sum TCC_MISS_sum of the launch alone (counters
#      never share a run with the trace domains, and FETCH_SIZE / WRITE_SIZE do not fit one pass)
# A run that fails or times out ends the script with its log tail and a non-zero exit: no further GPU step after it.
#   usage: [OUT_DIR=dir] bash tools/profile_gm.sh <tag> [gm_diag.py args]   -> $OUT_DIR/<tag>_*
#   (OUT_DIR defaults to build/profile_out, which git ignores)
set -o pipefail
TAG=${1:?tag}; shift
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${OUT_DIR:-build/profile_out}
mkdir -p $OUT
PROBE="python3 tools/probes/gm_diag.py $*"
step() { # name seconds command...
   n=$1; t=$2; shift 2
   timeout -k 10 $t "$@" > $OUT/${TAG}_$n.log 2>&1
   rc=$?
   echo "[gm] $n rc=$rc"
   if [ $rc -ne 0 ]; then
      echo "[gm] $n FAILED (rc $rc; 124 = timeout): last lines of its log" >&2
      tail -20 $OUT/${TAG}_$n.log >&2
      exit $rc
   fi
}
step diag 500 $PROBE --out $OUT/${TAG}_diag_qu30.json
step trace 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_trace -o t -- $PROBE --only-kernel --iters 20
step pmc_fetch 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/${TAG}_pmc_fetch -o f -- $PROBE --only-kernel --iters 6
step pmc_write 300 rocprofv3 --pmc WRITE_SIZE TCC_HIT_sum TCC_MISS_sum --output-format csv -d $OUT/${TAG}_pmc_write -o w -- $PROBE --only-kernel --iters 6
GM_OUT=$OUT GM_TAG=$TAG python3 - <<'PY'
import collections, csv, glob, json, os
out, tag = os.environ["GM_OUT"], os.environ["GM_TAG"]
vals = collections.defaultdict(list)
for sub in ("pmc_fetch", "pmc_write"):
    for f in glob.glob(f"{out}/{tag}_{sub}/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if "bolusVelocityKernel" in r["Kernel_Name"]:
                vals[r["Counter_Name"]].append(float(r["Counter_Value"]))
mean = {k: sum(v) / len(v) for k, v in vals.items()}
res = {"_note": "rocprofv3 --pmc of bolusVelocityKernel alone, means per launch; FETCH_SIZE (KB) x 1024 x 2 (gfx950 tallies "
                "128-byte requests at 64 B) + WRITE_SIZE (KB) x 1024", "launches_sampled": {k: len(v) for k, v in vals.items()},
       "counters_mean": mean}
if "FETCH_SIZE" in mean and "WRITE_SIZE" in mean:
    res["fetch_bytes_per_launch_x2"] = mean["FETCH_SIZE"] * 1024 * 2
    res["write_bytes_per_launch"] = mean["WRITE_SIZE"] * 1024
    res["hbm_bytes_per_launch"] = res["fetch_bytes_per_launch_x2"] + res["write_bytes_per_launch"]
stats = []
for f in glob.glob(f"{out}/{tag}_trace/**/*kernel_stats.csv", recursive=True):
    stats += [r for r in csv.DictReader(open(f)) if "bolusVelocityKernel" in r.get("Name", "")]
res["kernel_stats"] = stats
json.dump(res, open(f"{out}/{tag}_counters_qu30.json", "w"), indent=1)
print(json.dumps(res))
PY
