# Round-6 first GPU call: every GPU test (with the cfg4 eight-rank test), the cfg4 gloo
# rehearsal bench (8 ranks on one GPU, 2048 images), then the default bench line.
set -u
TAG=${1:-r06a}
cd "$GRAFT_REPO_ROOT"
LOGS=$(realpath -m "${LOGS:-bench_out}"); mkdir -p "$LOGS"  # LOGS=<dir>: where the outputs go
timeout -k 10 900 python -u -m pytest tests -x -v -m gpu -p no:cacheprovider \
  --timeout 120 --timeout-method thread > $LOGS/${TAG}_tests.log 2>&1
rc=$?
tail -3 $LOGS/${TAG}_tests.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python -u bench.py --full --gpus 8 --backend gloo --workload cfg4 --no-uniform \
  --no-multi --no-configs --no-cpu-baseline > $LOGS/${TAG}_bench_gloo8.json \
  2> $LOGS/${TAG}_bench_gloo8.err || exit $?
cat $LOGS/${TAG}_bench_gloo8.json
timeout -k 10 300 python -u bench.py --full --no-cpu-baseline > $LOGS/${TAG}_bench.json \
  2> $LOGS/${TAG}_bench.err || exit $?
cat $LOGS/${TAG}_bench.json
