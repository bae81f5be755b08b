# Iteration call: the -m gpu tests (TESTS=0 skips them), then the default bench line without
# the CPU leg.  Usage (via gpurun): bash tools/gpu_iter.sh <tag>
set -u
TAG=${1:-iter}
cd "$GRAFT_REPO_ROOT"
LOGS=$(realpath -m "${LOGS:-bench_out}"); mkdir -p "$LOGS"  # LOGS=<dir>: where the outputs go
if [ "${TESTS:-1}" = "1" ]; then
  timeout -k 10 900 python -u -m pytest tests -x -v -m gpu -p no:cacheprovider \
    --timeout 120 --timeout-method thread > $LOGS/${TAG}_tests.log 2>&1
  rc=$?
  tail -3 $LOGS/${TAG}_tests.log
  [ $rc -eq 0 ] || exit $rc
fi
timeout -k 10 300 python -u bench.py --full --no-cpu-baseline ${BENCH_ARGS:-} > $LOGS/${TAG}_bench.json \
  2> $LOGS/${TAG}_bench.err || exit $?
cat $LOGS/${TAG}_bench.json
