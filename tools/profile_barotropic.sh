#!/bin/bash
# BarotropicMode at QU30 size (tools/probes/barotropic_diag.py), two runs of their own, each bounded by timeout:
#   1. device-event timing of the split launches, of 30 sub-steps and of one fused RHS in the same process (no profiler)
#   2. rocprofv3 --kernel-trace --stats of the launches alone
# A run that fails or times out ends the script with its log tail and a non-zero exit: no further GPU step after it.
#   usage: [OUT_DIR=dir] [STEPS="diag trace"] bash tools/profile_barotropic.sh <tag> [barotropic_diag.py args]
#   -> $OUT_DIR/<tag>_*   (OUT_DIR defaults to build/profile_out, which git ignores)
NAME=barotropic
. "$(dirname "$0")/profile_lib.sh"
STEPS=${STEPS:-diag trace}
PROBE="python3 tools/probes/barotropic_diag.py $*"
case " $STEPS " in *" diag "*)
   step diag 500 $PROBE --out $OUT/${TAG}_diag_qu30.json
   cat $OUT/${TAG}_diag_qu30.json ;;
esac
case " $STEPS " in *" trace "*)
   trace $PROBE --only-kernels --iters 20
   kernel_stats btr ;;
esac
exit 0
