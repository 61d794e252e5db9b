#!/bin/bash
# One GPU session: parity tests, smoke, bench, rocprofv3 kernel trace.
# Every GPU step has its own time limit.  An ordinary test failure (pytest exit 1) lets the
# session go on to the bench; a crash, abort, fault or time-out (any other non-zero status)
# ends it there.
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT_DIR:-bench_out}  # where this script leaves its logs and profiles (ignored by git)
TAG=${1:-r01}
STEPS=${2:-all}
mkdir -p $OUT
export TMPDIR=/tmp

stop_unless_ok() {  # $1 = status, $2 = step name, $3 = allowed non-fatal status
  if [ "$1" -ne 0 ] && [ "$1" -ne "${3:-0}" ]; then
    echo "!! $2 ended with status $1: stopping"
    exit "$1"
  fi
}

if [[ $STEPS == all || $STEPS == *test* ]]; then
  echo "== pytest -m gpu"
  timeout -k 10 900 python3 -u -m pytest tests -m gpu -q -p no:cacheprovider --timeout 300 --timeout-method thread > $OUT/pytest_gpu_$TAG.log 2>&1
  rc=$?; tail -25 $OUT/pytest_gpu_$TAG.log; stop_unless_ok $rc pytest 1
  echo "== smoke"
  timeout -k 10 300 python3 -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$TAG.log 2>&1
  rc=$?; tail -3 $OUT/smoke_$TAG.log; stop_unless_ok $rc smoke 1
fi
if [[ $STEPS == all || $STEPS == *bench* ]]; then
  echo "== bench"
  timeout -k 10 600 python3 bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err
  rc=$?; cat $OUT/bench_$TAG.json; tail -5 $OUT/bench_$TAG.err; stop_unless_ok $rc bench
fi
if [[ $STEPS == all || $STEPS == *prof* ]]; then
  echo "== rocprofv3 kernel trace"
  timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o run -- \
    python3 bench.py --full --steps 2 --warmup 1 --cpu-sample 0 > $OUT/bench_prof_$TAG.json 2> $OUT/bench_prof_$TAG.err
  rc=$?; cat $OUT/bench_prof_$TAG.json; tail -5 $OUT/bench_prof_$TAG.err; stop_unless_ok $rc rocprofv3
  find $OUT/prof_$TAG -name "*stats*"
fi
if [[ $STEPS == all || $STEPS == *traffic* ]]; then
  echo "== PMC traffic"
  OUT_DIR=$OUT bash scripts/pmc_traffic.sh $TAG; stop_unless_ok $? traffic
fi
echo "== done"
