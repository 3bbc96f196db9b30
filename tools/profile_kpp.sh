#!/bin/bash
# Kpp at QU30 size (tools/probes/kpp_diag.py), four runs of their own, each bounded by timeout:
#   1. device-event timing of Kpp::compute and Kpp::applyNonLocalTracerFlux next to VertMix::computeVertMix (the same edge
#      gather over the same rows), alternating in one loop, every case twice (no profiler)
#   2. rocprofv3 --kernel-trace --stats of the launches alone
#   3. rocprofv3 --pmc FETCH_SIZE, 4. rocprofv3 --pmc WRITE_SIZE TCC_HIT_sum TCC_MISS_sum of the launches alone
#      (counters never share a run with the trace domains, and FETCH_SIZE / WRITE_SIZE do not fit one pass)
# A run that fails or times out ends the script with its log tail and a non-zero exit: no further GPU step after it.
#   usage: [OUT_DIR=dir] [ONLY_DIAG=1] bash tools/profile_kpp.sh <tag> [kpp_diag.py args]   -> $OUT_DIR/<tag>_*
#   (OUT_DIR defaults to build/profile_out, which git ignores; ONLY_DIAG=1 stops after run 1)
NAME=kpp
. "$(dirname "$0")/profile_lib.sh"
PROBE="python3 tools/probes/kpp_diag.py $*"
step diag 540 $PROBE --out $OUT/${TAG}_diag_qu30.json
[ -n "$ONLY_DIAG" ] && exit 0
trace $PROBE --only-kernels --iters 20
pmc_fetch $PROBE --only-kernels --iters 6
pmc_write $PROBE --only-kernels --iters 6
counters "rocprofv3 --pmc of the Kpp kernels and the coefficient kernel alone, means per launch; FETCH_SIZE (KB) x 1024 x 2 (gfx950 tallies 128-byte requests at 64 B) + WRITE_SIZE (KB) x 1024" kppComputeKernel kppNonLocalKernel vertMixCoeffKernel
