#!/bin/bash
# PressureGrad at QU30 size (tools/probes/pressure_grad_diag.py), four runs of their own, each bounded by timeout:
#   1. device-event timing of the kernel, the column pass, the plain and the layered RHS and RK4 step (no profiler)
#   2. rocprofv3 --kernel-trace --stats of the kernel alone
#   3. rocprofv3 --pmc FETCH_SIZE, 4. rocprofv3 --pmc WRITE_SIZE TCC_HIT_sum TCC_MISS_sum of the kernel alone (counters
#      never share a run with the trace domains, and FETCH_SIZE / WRITE_SIZE do not fit one pass)
# A run that fails or times out ends the script with its log tail and a non-zero exit: no further GPU step after it.
#   usage: [OUT_DIR=dir] bash tools/profile_pressure_grad.sh <tag> [pressure_grad_diag.py args]   -> $OUT_DIR/<tag>_*
#   (OUT_DIR defaults to build/profile_out, which git ignores)
NAME=pgrad
. "$(dirname "$0")/profile_lib.sh"
PROBE="python3 tools/probes/pressure_grad_diag.py $*"
step diag 500 $PROBE --out $OUT/${TAG}_diag_qu30.json
trace $PROBE --only-kernel --iters 20
pmc_fetch $PROBE --only-kernel --iters 6
pmc_write $PROBE --only-kernel --iters 6
counters "rocprofv3 --pmc of pressureGradKernel alone, means per launch; FETCH_SIZE (KB) x 1024 x 2 (gfx950 tallies 128-byte requests at 64 B) + WRITE_SIZE (KB) x 1024" --flat pressureGradKernel
