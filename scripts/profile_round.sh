#!/bin/bash
# Round evidence on one GPU: the full bench line (bench.py --full: cpu_baseline and
# companions), rocprofv3 kernel-trace stats of the plain run, and two separate PMC passes
# (FETCH_SIZE, WRITE_SIZE) for the HBM traffic of the main kernel.
# usage: scripts/profile_round.sh TAG [extra bench args]
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
O=${EVIDENCE_DIR:-evidence}  # where the records go (scripts/collect_evidence.sh files them under profiles/)
mkdir -p $O
export TMPDIR=/tmp
TAG=${1:-r01}; shift || true
EXTRA="$*"
fatal() { [ "$1" -ne 0 ]; }
timeout -k 10 420 python bench.py --full $EXTRA > $O/bench_$TAG.json 2> $O/bench_$TAG.err
rc=$?; echo "bench rc=$rc"; cat $O/bench_$TAG.json; tail -3 $O/bench_$TAG.err; fatal $rc && exit $rc
rm -rf $O/prof_$TAG $O/pmcf_$TAG $O/pmcw_$TAG
timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$TAG -o run -- \
    python3 bench.py --cpu-seconds 0 --f32-steps 0 --c5-steps 0 --c2-steps 0 --c4-steps 0 --demod-steps 0 $EXTRA > $O/prof_$TAG.log 2>&1
rc=$?; echo "rocprof stats rc=$rc"; fatal $rc && { tail -5 $O/prof_$TAG.log; exit $rc; }
find $O/prof_$TAG -name "*kernel_stats.csv" -exec cat {} \;
SHORT="--cpu-seconds 0 --f32-steps 0 --c5-steps 0 --c2-steps 0 --c4-steps 0 --demod-steps 0 --steps 2 --warmup 1 --calls-per-step 4"
timeout -k 10 420 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmcf_$TAG -o run -- \
    python3 bench.py $SHORT $EXTRA > $O/pmcf_$TAG.log 2>&1
rc=$?; echo "pmc fetch rc=$rc"; fatal $rc && { tail -5 $O/pmcf_$TAG.log; exit $rc; }
timeout -k 10 420 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/pmcw_$TAG -o run -- \
    python3 bench.py $SHORT $EXTRA > $O/pmcw_$TAG.log 2>&1
rc=$?; echo "pmc write rc=$rc"; fatal $rc && { tail -5 $O/pmcw_$TAG.log; exit $rc; }
F=$(find $O/pmcf_$TAG -name "*counter_collection.csv" | head -1)
W=$(find $O/pmcw_$TAG -name "*counter_collection.csv" | head -1)
python3 scripts/pmc_summary.py "$F" "$W" s8_65536_500 fft_wide_kernel $O/pmc_traffic_$TAG.json "profiles/$TAG" || true
exit 0
