#!/bin/bash
# The forced VertMix solves at QU30 size (tools/probes/vert_mix_forcing_diag.py), two runs of their own, each bounded by
# timeout:
#   1. device-event timing: forced against unforced launches alternating in one process, VertMixStep.apply, an RK4 step
#      with and without the stepper hook (no profiler)
#   2. rocprofv3 --kernel-trace --stats of the solves alone
# A run that fails or times out ends the script with its log tail and a non-zero exit: no further GPU step after it.
#   usage: [OUT_DIR=dir] bash tools/profile_vert_mix_forcing.sh <tag> [vert_mix_forcing_diag.py args]   -> $OUT_DIR/<tag>_*
#   (OUT_DIR defaults to build/profile_out, which git ignores)
set -o pipefail
TAG=${1:?tag}; shift
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${OUT_DIR:-build/profile_out}
mkdir -p $OUT
PROBE="python3 tools/probes/vert_mix_forcing_diag.py $*"
step() { # name seconds command...
   n=$1; t=$2; shift 2
   timeout -k 10 $t "$@" > $OUT/${TAG}_$n.log 2>&1
   rc=$?
   echo "[vertmixforcing] $n rc=$rc"
   if [ $rc -ne 0 ]; then
      echo "[vertmixforcing] $n FAILED (rc $rc; 124 = timeout): last lines of its log" >&2
      tail -20 $OUT/${TAG}_$n.log >&2
      exit $rc
   fi
}
step diag 500 $PROBE --out $OUT/${TAG}_diag_qu30.json &&
step trace 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_trace -o t -- $PROBE --only-kernels --iters 20 &&
find $OUT/${TAG}_trace -name '*kernel_stats.csv' -exec grep -h -E '^"?Name|implicitMix' {} \; > $OUT/${TAG}_kernel_stats_qu30.csv
cat $OUT/${TAG}_diag_qu30.json
