#!/bin/bash
# VertRemap at QU30 size (tools/probes/vert_remap_diag.py), four runs of their own, each bounded by timeout:
#   1. device-event timing of remap at each order (PCM, PLM, PPM), alternating in one loop, and of whole Split-Explicit
#      steps without and with the remap attached, alternating in one loop (no profiler)
#   2. rocprofv3 --kernel-trace --stats of the remap launches alone
#   3. rocprofv3 --pmc FETCH_SIZE, 4. rocprofv3 --pmc WRITE_SIZE TCC_HIT_sum TCC_MISS_sum of the remap launches alone
#      (counters never share a run with the trace domains, and FETCH_SIZE / WRITE_SIZE do not fit one pass)
# A run that fails or times out ends the script with its log tail and a non-zero exit: no further GPU step after it.
#   usage: [OUT_DIR=dir] [ONLY_DIAG=1] bash tools/profile_vert_remap.sh <tag> [vert_remap_diag.py args]   -> $OUT_DIR/<tag>_*
#   (OUT_DIR defaults to build/profile_out, which git ignores; ONLY_DIAG=1 stops after run 1)
set -o pipefail
TAG=${1:?tag}; shift
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${OUT_DIR:-build/profile_out}
mkdir -p $OUT
PROBE="python3 tools/probes/vert_remap_diag.py $*"
step() { # name seconds command...
   n=$1; t=$2; shift 2
   timeout -k 10 $t "$@" > $OUT/${TAG}_$n.log 2>&1
   rc=$?
   echo "[vert_remap] $n rc=$rc"
   if [ $rc -ne 0 ]; then
      echo "[vert_remap] $n FAILED (rc $rc; 124 = timeout): last lines of its log" >&2
      tail -20 $OUT/${TAG}_$n.log >&2
      exit $rc
   fi
}
step diag 540 $PROBE --out $OUT/${TAG}_diag_qu30.json
[ -n "$ONLY_DIAG" ] && exit 0
step trace 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_trace -o t -- $PROBE --only-kernels --iters 10
step pmc_fetch 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/${TAG}_pmc_fetch -o f -- $PROBE --only-kernels --iters 4
step pmc_write 300 rocprofv3 --pmc WRITE_SIZE TCC_HIT_sum TCC_MISS_sum --output-format csv -d $OUT/${TAG}_pmc_write -o w -- $PROBE --only-kernels --iters 4
VR_OUT=$OUT VR_TAG=$TAG python3 - <<'PY'
import collections, csv, glob, json, os
out, tag = os.environ["VR_OUT"], os.environ["VR_TAG"]
KERNELS = ("vertRemapCellKernel", "vertRemapEdgeKernel", "vertRemapAdoptKernel")
res = {"_note": "rocprofv3 --pmc of the VertRemap kernels alone (the three orders together), means per launch; FETCH_SIZE "
                "(KB) x 1024 x 2 (gfx950 tallies 128-byte requests at 64 B) + WRITE_SIZE (KB) x 1024", "kernels": {}}
for kern in KERNELS:
    vals = collections.defaultdict(list)
    for sub in ("pmc_fetch", "pmc_write"):
        for f in glob.glob(f"{out}/{tag}_{sub}/**/*counter_collection.csv", recursive=True):
            for r in csv.DictReader(open(f)):
                if kern in r["Kernel_Name"]:
                    vals[r["Counter_Name"]].append(float(r["Counter_Value"]))
    mean = {k: sum(v) / len(v) for k, v in vals.items()}
    one = {"launches_sampled": {k: len(v) for k, v in vals.items()}, "counters_mean": mean}
    if "FETCH_SIZE" in mean and "WRITE_SIZE" in mean:
        one["fetch_bytes_per_launch_x2"] = mean["FETCH_SIZE"] * 1024 * 2
        one["write_bytes_per_launch"] = mean["WRITE_SIZE"] * 1024
        one["hbm_bytes_per_launch"] = one["fetch_bytes_per_launch_x2"] + one["write_bytes_per_launch"]
    stats = []
    for f in glob.glob(f"{out}/{tag}_trace/**/*kernel_stats.csv", recursive=True):
        stats += [r for r in csv.DictReader(open(f)) if kern in r.get("Name", "")]
    one["kernel_stats"] = stats
    res["kernels"][kern] = one
json.dump(res, open(f"{out}/{tag}_counters_qu30.json", "w"), indent=1)
print(json.dumps(res))
PY
