#!/bin/bash
# VertAdv at QU30 size (tools/probes/vert_adv_diag.py), two runs of their own, each bounded by timeout:
#   1. device-event timing of each launch, of the plain and the attached RHS and RK4 step (no profiler)
#   2. rocprofv3 --kernel-trace --stats of the launches alone
# A run that fails or times out ends the script with its log tail and a non-zero exit: no further GPU step after it.
#   usage: [OUT_DIR=dir] bash tools/profile_vert_adv.sh <tag> [vert_adv_diag.py args]   -> $OUT_DIR/<tag>_*
#   (OUT_DIR defaults to build/profile_out, which git ignores)
NAME=vertadv
. "$(dirname "$0")/profile_lib.sh"
PROBE="python3 tools/probes/vert_adv_diag.py $*"
step diag 500 $PROBE --out $OUT/${TAG}_diag_qu30.json
trace $PROBE --only-kernels --iters 20
kernel_stats vertAdv
cat $OUT/${TAG}_diag_qu30.json
