#!/bin/bash
# One GPU session: parity tests, smoke, bench (every leg: --full), rocprofv3 kernel stats.
# Each GPU step has its own time limit; a crash/timeout/fault (rc >= 124 or signal) stops the
# session, test failures (rc 1) do not.  Logs and the profile go to $OUT (default session_out/):
# set OUT to the folder pmc_traffic.py summarises when its kernel-stats table is wanted.
set -u
cd "$(dirname "$0")/.."
OUT=${OUT:-session_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
STEPS=${STEPS:-200}
run() {  # name timeout cmd...
  local name=$1 t=$2; shift 2
  echo "=== $name: $*" | tee -a "$OUT/session.log"
  timeout -k 10 "$t" "$@" > "$OUT/$name.log" 2>&1
  local rc=$?
  echo "=== $name rc=$rc" | tee -a "$OUT/session.log"
  tail -5 "$OUT/$name.log"
  if [ $rc -ge 124 ] || [ $rc -gt 128 ] || [ $rc -eq 134 ] || [ $rc -eq 139 ]; then
    echo "stopping after $name (rc=$rc)"; exit $rc
  fi
  return 0
}
if [ "${SKIP_TESTS:-0}" != 1 ]; then
  run pytest_gpu 600 python -m pytest tests -m gpu -q -x -p no:cacheprovider
  run smoke 300 python -c "import __graft_entry__ as g; g.smoke()"
fi
run bench 600 python bench.py --full --steps "$STEPS" --warmup 20 --cpu-seconds 10
if [ "${SKIP_PROF:-0}" != 1 ]; then
  run rocprof 600 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run --output-format csv -- python bench.py --full --steps 100 --warmup 10 --no-cpu-baseline
fi
