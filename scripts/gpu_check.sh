#!/bin/bash
# One GPU session: smoke, GPU parity tests, bench, rocprofv3 kernel stats.
# Stops at the first step that faults / aborts / times out (exit >= 2 from
# pytest counts as a hard failure too); assertion failures in pytest (exit 1)
# are recorded and the measurement steps still run.  Output: $OUT_DIR
# (default bench_out/ in the repository).
set -u
R="$(cd "$(dirname "$0")/.." && pwd)"
cd "$R"
O="$R/${OUT_DIR:-bench_out}"
mkdir -p "$O"
export TMPDIR=/tmp
TAG=${TAG:-r01}
STEPS=${STEPS:-20}
hard_fail() { echo "hard failure ($1) in $2; stopping"; exit "$1"; }

timeout -k 10 240 python -c "import __graft_entry__ as g; g.smoke()" > "$O/smoke.log" 2>&1
rc=$?; echo "smoke rc=$rc"; [ $rc -ne 0 ] && { tail -30 "$O/smoke.log"; [ $rc -ge 2 ] && hard_fail $rc smoke; }

if [ "${SKIP_TESTS:-0}" != "1" ]; then
  timeout -k 10 600 python -m pytest tests -x -q -m gpu ${PYTEST_ARGS:-} > "$O/pytest_gpu.log" 2>&1
  rc=$?; echo "pytest rc=$rc"; tail -15 "$O/pytest_gpu.log"
  [ $rc -ge 2 ] && hard_fail $rc pytest
fi

# the whole line (--full: host path, roofline, Texture leg, CPU baseline)
timeout -k 10 300 python bench.py --full --steps $STEPS --warmup 5 > "$O/bench_$TAG.json" 2> "$O/bench_$TAG.err"
rc=$?; echo "bench rc=$rc"; cat "$O/bench_$TAG.json"; [ $rc -ne 0 ] && { tail -20 "$O/bench_$TAG.err"; hard_fail $rc bench; }

if [ "${SKIP_PROF:-0}" != "1" ]; then
  cd /tmp
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$O/prof_$TAG" -o run --output-format csv -- \
      python "$R/bench.py" --full --steps $STEPS --warmup 5 --no-cpu-baseline > "$O/prof_$TAG.log" 2>&1
  rc=$?; echo "rocprof rc=$rc"; [ $rc -ne 0 ] && { tail -20 "$O/prof_$TAG.log"; hard_fail $rc rocprof; }
  find "$O/prof_$TAG" -name "*stats*" | head
fi
echo done
