#!/bin/bash
# SplitExplicitStepper at QU30 size (tools/probes/split_explicit_diag.py): device-event timing of the three BarotropicMode
# calls of the step, of the group calls of steps 6 and 7, of one Split-Explicit step, one stage-fused RungeKutta4 step and
# one fused RHS in the same process (no profiler), bounded by timeout.
# A run that fails or times out ends the script with its log tail and a non-zero exit: no further GPU step after it.
#   usage: [OUT_DIR=dir] bash tools/profile_split_explicit.sh <tag> [split_explicit_diag.py args]
#   -> $OUT_DIR/<tag>_*   (OUT_DIR defaults to build/profile_out, which git ignores)
NAME=split-explicit
. "$(dirname "$0")/profile_lib.sh"
step diag 500 python3 tools/probes/split_explicit_diag.py "$@" --out $OUT/${TAG}_diag_qu30.json
cat $OUT/${TAG}_diag_qu30.json
