#!/bin/bash
# One gpurun session: GPU tests, a short bench, and a rocprofv3 kernel-trace
# summary.  Each GPU step has its own time limit; the script stops at the
# first step that crashes, aborts or times out (exit 124/134/137/139), and
# carries on past plain test failures (exit 1) so the bench still reports.
set -u
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}   # where the logs and records go
mkdir -p "$OUT"
export TMPDIR=/tmp
STEPS=${STEPS:-tests bench prof}
fatal() { case "$1" in 124|134|137|139) return 0;; *) return 1;; esac; }
for s in $STEPS; do
  case $s in
    tests)
      timeout -k 10 900 python -m pytest tests -m gpu -x -q -p no:cacheprovider > $OUT/pytest_gpu.log 2>&1
      rc=$?; echo "pytest gpu rc=$rc"; tail -5 $OUT/pytest_gpu.log
      fatal $rc && exit $rc ;;
    smoke)
      timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1
      rc=$?; echo "smoke rc=$rc"; tail -3 $OUT/smoke.log
      fatal $rc && exit $rc ;;
    bench)
      timeout -k 10 900 python bench.py --full ${BENCH_ARGS:-} > $OUT/bench.log 2>&1
      rc=$?; echo "bench rc=$rc"; tail -3 $OUT/bench.log
      fatal $rc && exit $rc ;;
    prof)
      timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof -o run --output-format csv \
        -- python bench.py --steps 4 --warmup 1 --no-cpu-baseline --no-roofline > $OUT/prof.log 2>&1
      rc=$?; echo "prof rc=$rc"; tail -3 $OUT/prof.log
      fatal $rc && exit $rc ;;
  esac
done
exit 0
