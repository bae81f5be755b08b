# One GPU call for a round checkpoint: parity tests, smoke, the default bench line, then
# the rocprofv3 kernel trace + PMC passes (tools/gpu_profile.sh).  Every GPU step has its
# own time limit and the chain stops at the first failure.
# Usage (via gpurun): bash tools/gpu_round.sh <tag>;  then here: python tools/prof_summary.py <tag>
set -u
TAG=${1:-r01c}
cd "$GRAFT_REPO_ROOT"
LOGS=$(realpath -m "${LOGS:-bench_out}"); mkdir -p "$LOGS"  # LOGS=<dir>: where the outputs go
timeout -k 10 540 python -u -m pytest tests -x -q -m gpu -p no:cacheprovider \
  --timeout 120 --timeout-method thread > $LOGS/${TAG}_tests.log 2>&1
rc=$?
tail -3 $LOGS/${TAG}_tests.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 180 python -u -c "import __graft_entry__ as g; g.smoke()" > $LOGS/${TAG}_smoke.log 2>&1 || exit $?
tail -1 $LOGS/${TAG}_smoke.log
timeout -k 10 300 python -u bench.py --full > $LOGS/${TAG}_bench.json 2> $LOGS/${TAG}_bench.err || exit $?
cat $LOGS/${TAG}_bench.json
[ "${PROFILE:-1}" = "1" ] && bash tools/gpu_profile.sh "$TAG"
true
