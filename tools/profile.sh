#!/bin/bash
# The round's profiles (run on the GPU box: `tools/profile.sh r09 [counters|all]`), ONE refresh for the round's kept code.
#   counters  the passes the committed figures of bench.py rest on: HBM traffic of the headline batch (FETCH_SIZE / WRITE_SIZE in separate passes,
#             as MI355X_MICROARCH.md prescribes) and one SQ pass each for the headline batch (64 distinct streams), the 1 024-stream batch (throughput
#             regime), stream mode and the 12 800-capture scanner batch -> <tag>_pmc_traffic.json, <tag>_sq_counters.csv, <tag>_valu_per_step.json,
#             stamped with the source hash (tests/test_abi_cpu.py and bench.py refuse a summary of other sources).  What every change under csrc/ needs.
#   all       (default) plus rocprofv3 kernel stats (of the headline loop as it runs, calls in flight, and of the same loop fenced behind every step:
#             the per-kernel figures of bench.py's event pass), the other regimes' stats / traffic / SQ tables, the scanner timeline, the N > 1 step
#             cost on one rank (tools/dist_cost.py) and the clock / LDS micro-benchmark.
# Every step runs under a time limit of its own and the first step that fails, faults or runs into its limit ENDS the script: nothing is started on a
# GPU after a step that did not end well.  Counter (--pmc) passes are runs of their own, never combined with tracing.
# Raw .db files land in $GSMCAL_PROFILE_OUT (default: profile_out/ in the repository root); profiles/rocpd_summary.py turns them into the small files kept under profiles/.
set -u
RT=${1:-r06}     # round tag: prefixes every file written under profiles/ and $O/
MODE=${2:-all}
LIMIT=${GSMCAL_PROFILE_STEP_LIMIT:-300}   # seconds per step
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=${GSMCAL_PROFILE_OUT:-$R/profile_out}   # raw outputs and logs (absolute path, or relative to the repository root); kept out of git
case $O in /*) ;; *) O=$R/$O;; esac
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
export GSMCAL_BENCH_NO_VARIANTS=1     # (the headline loop only: no depth-2 / one-buffer variants behind it)
B="python3 $R/bench.py --full --no-cpu-baseline --no-sub --no-kernel-events --cache-streams /tmp/gsmcal_streams"
CAL="$B --steps 20 --warmup 3"
CALC="$CAL --prewarm-steps 0"     # counter passes: the counters do not depend on the clock state, and 256 fewer steps keep the .db files small
BIG="$B --steps 10 --warmup 3 --streams 1024 --prewarm-steps 20"
STR="$B --steps 10 --warmup 3 --mode stream --prewarm-steps 20"
SCAN="$B --workload scan --streams 12800 --frames 64 --distinct 32 --steps 6 --warmup 2"
SQ="SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_WAIT_ANY"
# step <name> <command...>: the command under its own time limit, stdout to $O/<name>.out, stderr to $O/<name>.log; anything but exit
# status 0 ends the script
step() {
    local name=$1; shift
    echo "[profile] $name"
    timeout -k 10 $LIMIT "$@" > $O/$name.out 2> $O/$name.log
    local rc=$?
    if [ $rc -ne 0 ]; then
        echo "[profile] $name ended with status $rc: stopping here (nothing further is started)"; tail -5 $O/$name.log
        exit $rc
    fi
}
run() { local name=$1; shift; step $name rocprofv3 "$@"; }
step ${RT}_bench_n1_noprof $CAL      # (fills the stream cache; also the unprofiled line)
cp $O/${RT}_bench_n1_noprof.out $O/${RT}_bench_n1_noprof.json
run ${RT}_fetch         --pmc FETCH_SIZE -d $O/${RT}_fetch -o ${RT} -- $CALC
run ${RT}_write         --pmc WRITE_SIZE -d $O/${RT}_write -o ${RT} -- $CALC
run ${RT}_sq            --pmc $SQ -d $O/${RT}_sq -o ${RT} -- $CALC
run ${RT}_big_sq        --pmc $SQ -d $O/${RT}_big_sq -o ${RT} -- $BIG
run ${RT}_str_sq        --pmc $SQ -d $O/${RT}_str_sq -o ${RT} -- $STR
run ${RT}_scan_sq       --pmc $SQ -d $O/${RT}_scan_sq -o ${RT} -- $SCAN
if [ "$MODE" = all ]; then
run ${RT}_stats         --kernel-trace --stats -d $O/${RT}_stats -o ${RT} -- $CAL
run ${RT}_iso_stats     --kernel-trace --stats -d $O/${RT}_iso_stats -o ${RT} -- $CAL --one-in-flight   # the same kernels, each with the GPU to itself
run ${RT}_big_stats     --kernel-trace --stats -d $O/${RT}_big_stats -o ${RT} -- $BIG
run ${RT}_str_stats     --kernel-trace --stats -d $O/${RT}_str_stats -o ${RT} -- $STR
run ${RT}_scan_stats    --kernel-trace --stats -d $O/${RT}_scan_stats -o ${RT} -- $SCAN
run ${RT}_scan_fetch    --pmc FETCH_SIZE -d $O/${RT}_scan_fetch -o ${RT} -- $SCAN
run ${RT}_scan_write    --pmc WRITE_SIZE -d $O/${RT}_scan_write -o ${RT} -- $SCAN
fi
cd $R
P="python3 profiles/rocpd_summary.py"
db() { find $O/$1 -name '*.db' | head -1; }
set -e
$P pmc $(db ${RT}_fetch) $(db ${RT}_write) profiles/${RT}_pmc_traffic.json 64 1020000
$P sq $(db ${RT}_sq) profiles/${RT}_sq_counters.csv
$P valu profiles/${RT}_valu_per_step.json calib_64=$(db ${RT}_sq):1 calib_1024=$(db ${RT}_big_sq):4 stream_mode_64=$(db ${RT}_str_sq):1 scan_12800=$(db ${RT}_scan_sq):s8
if [ "$MODE" = all ]; then
$P stats $(db ${RT}_stats) profiles/${RT}_kernel_stats.csv 3
$P stats $(db ${RT}_iso_stats) profiles/${RT}_kernel_stats_one_call_at_a_time.csv 3
$P stats $(db ${RT}_big_stats) profiles/${RT}_streams1024_kernel_stats.csv 3
$P sq $(db ${RT}_big_sq) profiles/${RT}_streams1024_sq_counters.csv
$P stats $(db ${RT}_str_stats) profiles/${RT}_stream_mode_kernel_stats.csv 3
$P sq $(db ${RT}_str_sq) profiles/${RT}_stream_mode_sq_counters.csv
$P stats $(db ${RT}_scan_stats) profiles/${RT}_scan12800_kernel_stats.csv 2
$P pmc $(db ${RT}_scan_fetch) $(db ${RT}_scan_write) profiles/${RT}_scan12800_pmc_traffic.json 12800 640000
$P sq $(db ${RT}_scan_sq) profiles/${RT}_scan12800_sq_counters.csv
$P timeline $(db ${RT}_scan_stats) profiles/${RT}_scan12800_timeline.csv 72
fi
# which kernels these counters describe: the source hash (bench.py and the CPU suite refuse a summary of other sources) and the
# commit the tree was at when it was sent to the GPU box (written into profiles/.tree_commit before the call; the box has no .git)
python3 - profiles/${RT}_pmc_traffic.json profiles/${RT}_scan12800_pmc_traffic.json profiles/${RT}_valu_per_step.json <<'PY'
import json, os, sys
sys.path.insert(0, os.getcwd())
import gsmcal
h = gsmcal.build.csrc_hash()
commit = open("profiles/.tree_commit").read().strip() if os.path.exists("profiles/.tree_commit") else "unknown"
for f in sys.argv[1:]:
    if os.path.exists(f):
        d = json.load(open(f))
        d["csrc_sha256"] = h
        d["git_commit"] = commit
        json.dump(d, open(f, "w"), indent=1)
PY
set +e
mkdir -p $O/profiles_${RT} && cp profiles/${RT}_* $O/profiles_${RT}/     # (the summaries so far: kept even if a step below ends the script)
if [ "$MODE" = all ]; then
step ${RT}_dist_cost python3 tools/dist_cost.py
cp $O/${RT}_dist_cost.out profiles/${RT}_dist_cost.json
step ${RT}_clock_build /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 tools/micro/clock_fp64.hip -o /tmp/clock_fp64   # (built here: no binary in the tree)
step ${RT}_clock_lds_microbench /tmp/clock_fp64
cat $O/${RT}_clock_lds_microbench.out $O/${RT}_clock_lds_microbench.log > profiles/${RT}_clock_lds_microbench.txt
cp profiles/${RT}_* $O/profiles_${RT}/
fi
# the raw databases stay on the box (only small files travel back); the summaries above are what is kept
rm -rf $O/${RT}_stats $O/${RT}_iso_stats $O/${RT}_fetch $O/${RT}_write $O/${RT}_sq $O/${RT}_big_stats $O/${RT}_big_sq $O/${RT}_str_stats $O/${RT}_str_sq $O/${RT}_scan_stats $O/${RT}_scan_fetch $O/${RT}_scan_write $O/${RT}_scan_sq
ls -la profiles/ | grep ${RT}_
