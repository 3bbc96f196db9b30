#!/bin/bash
# BarotropicMode at QU30 size (tools/probes/barotropic_diag.py), two runs of their own, each bounded by timeout:
#   1. device-event timing of the split launches, of 30 sub-steps and of one fused RHS in the same process (no profiler)
#   2. rocprofv3 --kernel-trace --stats of the launches alone
# A run that fails or times out ends the script with its log tail and a non-zero exit: no further GPU step after it.
#   usage: [OUT_DIR=dir] [STEPS="diag trace"] bash tools/profile_barotropic.sh <tag> [barotropic_diag.py args]
#   -> $OUT_DIR/<tag>_*   (OUT_DIR defaults to build/profile_out, which git ignores)
set -o pipefail
TAG=${1:?tag}; shift
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${OUT_DIR:-build/profile_out}
STEPS=${STEPS:-diag trace}
mkdir -p $OUT
PROBE="python3 tools/probes/barotropic_diag.py $*"
step() { # name seconds command...
   n=$1; t=$2; shift 2
   timeout -k 10 $t "$@" > $OUT/${TAG}_$n.log 2>&1
   rc=$?
   echo "[barotropic] $n rc=$rc"
   if [ $rc -ne 0 ]; then
      echo "[barotropic] $n FAILED (rc $rc; 124 = timeout): last lines of its log" >&2
      tail -20 $OUT/${TAG}_$n.log >&2
      exit $rc
   fi
}
case " $STEPS " in *" diag "*)
   step diag 500 $PROBE --out $OUT/${TAG}_diag_qu30.json
   cat $OUT/${TAG}_diag_qu30.json ;;
esac
case " $STEPS " in *" trace "*)
   step trace 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_trace -o t -- $PROBE --only-kernels --iters 20
   find $OUT/${TAG}_trace -name '*kernel_stats.csv' -exec grep -h -E '^"?Name|btr' {} \; > $OUT/${TAG}_kernel_stats_qu30.csv ;;
esac
exit 0
