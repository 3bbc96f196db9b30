# Sourced by the tools/profile_*.sh scripts (and tools/pmc_diag.sh), after NAME -- the label of the script's lines -- and,
# where the script's file names carry one, LOG -- a prefix of its log and trace names -- are set:
#   . "$(dirname "$0")/profile_lib.sh"
# Takes <tag> off the script's arguments, moves to the repository root and makes $OUT (OUT_DIR, by default
# build/profile_out, which git ignores).  Everything that uses the GPU goes through step, each under a time limit of its own:
#   step <name> <seconds> <command...>   log in $OUT/<tag>_<LOG><name>.log; prints "[NAME] <name> rc=..."; a command that
#                                        fails or times out ends the script with its log tail and that status, so that no
#                                        further GPU step starts after it
# The three profiler steps are three runs: counters never share a run with a trace domain, FETCH_SIZE and WRITE_SIZE do not
# fit one pass, and the program goes after "--".
#   trace <command...>       rocprofv3 --kernel-trace --stats                     -> $OUT/<tag>_<LOG>trace
#   pmc_fetch <command...>   rocprofv3 --pmc FETCH_SIZE                           -> $OUT/<tag>_pmc_fetch
#   pmc_write <command...>   rocprofv3 --pmc WRITE_SIZE TCC_HIT_sum TCC_MISS_sum  -> $OUT/<tag>_pmc_write
#   counters <note> <kernel...>   condenses the three into $OUT/<tag>_counters_qu30.json (tools/summarise_profile.py)
#   kernel_stats <pattern>   the rows of the trace's --stats table that match, with its header -> <tag>_kernel_stats_qu30.csv
set -o pipefail
TAG=${1:?tag}; shift
cd "$(dirname "${BASH_SOURCE[0]}")/.."
export TMPDIR=/tmp
OUT=${OUT_DIR:-build/profile_out}
mkdir -p $OUT
step() {
   local n=$1 t=$2; shift 2
   local log=$OUT/${TAG}_${LOG}$n.log
   timeout -k 10 $t "$@" > $log 2>&1
   local rc=$?
   echo "[$NAME] $n rc=$rc"
   if [ $rc -ne 0 ]; then
      echo "[$NAME] $n FAILED (rc $rc; 124 = timeout): last lines of its log" >&2
      tail -20 $log >&2
      exit $rc
   fi
}
trace() { step trace 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_${LOG}trace -o t -- "$@"; }
pmc_fetch() { step pmc_fetch 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/${TAG}_pmc_fetch -o f -- "$@"; }
pmc_write() { step pmc_write 300 rocprofv3 --pmc WRITE_SIZE TCC_HIT_sum TCC_MISS_sum --output-format csv -d $OUT/${TAG}_pmc_write -o w -- "$@"; }
counters() { python3 tools/summarise_profile.py kernels --out-dir $OUT --tag $TAG --note "$@"; }
kernel_stats() { find $OUT/${TAG}_trace -name '*kernel_stats.csv' -exec grep -h -E "^\"?Name|$1" {} \; > $OUT/${TAG}_kernel_stats_qu30.csv; }
