#!/bin/bash
# The forced VertMix solves at QU30 size (tools/probes/vert_mix_forcing_diag.py), two runs of their own, each bounded by
# timeout:
#   1. device-event timing: forced against unforced launches alternating in one process, VertMixStep.apply, an RK4 step
#      with and without the stepper hook (no profiler)
#   2. rocprofv3 --kernel-trace --stats of the solves alone
# A run that fails or times out ends the script with its log tail and a non-zero exit: no further GPU step after it.
#   usage: [OUT_DIR=dir] bash tools/profile_vert_mix_forcing.sh <tag> [vert_mix_forcing_diag.py args]   -> $OUT_DIR/<tag>_*
#   (OUT_DIR defaults to build/profile_out, which git ignores)
NAME=vertmixforcing
. "$(dirname "$0")/profile_lib.sh"
PROBE="python3 tools/probes/vert_mix_forcing_diag.py $*"
step diag 500 $PROBE --out $OUT/${TAG}_diag_qu30.json
trace $PROBE --only-kernels --iters 20
kernel_stats implicitMix
cat $OUT/${TAG}_diag_qu30.json
