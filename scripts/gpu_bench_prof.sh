# Default bench (the driver's command) + rocprofv3 kernel-trace stats of the same workload.
# PROF_TAG names the output directories (gpurun_out/<tag>/...).
set -o pipefail
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
TAG=${PROF_TAG:-prof}
mkdir -p gpurun_out/$TAG
OUT=${TFG_OUT_DIR:-bench_out}/$TAG; mkdir -p $OUT  # the bench lines and traces of this script
echo "== smoke"
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > gpurun_out/$TAG/smoke.log 2>&1; rc=$?; echo "smoke rc=$rc"; tail -3 gpurun_out/$TAG/smoke.log
[ $rc -eq 0 ] || exit $rc
echo "== bench default"
timeout -k 10 600 python bench.py --full > $OUT/bench_default.log 2>&1; rc=$?; echo "bench rc=$rc"; tail -1 $OUT/bench_default.log
[ $rc -eq 0 ] || exit $rc
echo "== rocprof kernel trace"
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/trace -o run --output-format csv -- python bench.py --full --no-cpu-baseline > $OUT/trace.log 2>&1; rc=$?; echo "prof rc=$rc"
exit $rc
