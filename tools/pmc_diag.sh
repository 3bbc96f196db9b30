#!/bin/bash
# Diagnostic PMC passes for the RHS kernels, each in its own bench.py run under rocprofv3 (counters never share a run with
# the trace domains; a pass holds at most what one hardware block has slots for -- more aborts rocprofv3 with signal 6,
# "exceeds the capabilities of the hardware"), bounded by timeout.  A pass that fails or times out ends the script with
# its log tail and a non-zero exit: no further GPU step after a failed one.
#   sq      what the waves spend their cycles on (SQ_WAIT_ANY = parked at s_waitcnt, SQ_WAIT_INST_ANY = issue stall,
#           SQ_ACTIVE_INST_ANY = issuing; MI355X_MICROARCH.md "rocprofv3 PMC slots")
#   ta-tcp  texture-addresser / L1 path (four passes of two counters of one block)
#   usage (through gpurun): bash tools/pmc_diag.sh <tag> <sq|ta-tcp|all> [bench.py args]      (one script for the former
#   pmc_diag.sh + pmc_diag2.sh; a variant build is selected with OMEGA_AMD_LIB=.../libomega_amd_x.so in the environment)
NAME=diag
OUT=gpurun_out
OUT_DIR=$OUT
. "$(dirname "$0")/profile_lib.sh"
MODE=${1:?sq|ta-tcp|all}; shift
ARGS="--full --steps 4 --warmup 1 --rk4-steps 0 --no-cpu-baseline --no-live-traffic --realistic none $*"
PASSES=""
pass() { # name counters...
   local n=$1; shift
   step $n 150 rocprofv3 --pmc "$@" --output-format csv -d $OUT/${TAG}_$n -o p -- python3 bench.py $ARGS
   PASSES="$PASSES $n"
}
if [ "$MODE" = sq ] || [ "$MODE" = all ]; then
   pass sq SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_VMEM SQ_INSTS_VALU GRBM_GUI_ACTIVE
fi
if [ "$MODE" = ta-tcp ] || [ "$MODE" = all ]; then
   pass ta1 TA_BUSY_avr TA_BUFFER_TOTAL_CYCLES_sum GRBM_GUI_ACTIVE
   pass ta2 TA_ADDR_STALLED_BY_TC_CYCLES_sum TA_DATA_STALLED_BY_TC_CYCLES_sum GRBM_GUI_ACTIVE
   pass tcp1 TCP_PENDING_STALL_CYCLES_sum TCP_TCP_TA_DATA_STALL_CYCLES_sum GRBM_GUI_ACTIVE
   pass tcp2 TCP_TCC_READ_REQ_sum TCP_TOTAL_CACHE_ACCESSES_sum GRBM_GUI_ACTIVE
fi
python3 tools/summarise_profile.py passes --out-dir $OUT --tag $TAG $PASSES
