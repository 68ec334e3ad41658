#!/bin/bash
# GPU parity suite (one process, per-test timeout), then the full bench line (bench.py --full:
# round-trip comparison, whole-stream oracle check, CPU baseline).
# Logs go to $OUT (default: run_out/ in the repository root).
cd "$(dirname "$0")/.."
OUT=${OUT:-run_out}
mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread ${PYTEST_ARGS} > "$OUT/pytest_gpu.log" 2>&1 || { tail -40 "$OUT/pytest_gpu.log"; exit 1; }
tail -3 "$OUT/pytest_gpu.log"
if [ -z "$SKIP_BENCH" ]; then
timeout -k 10 600 python -u bench.py --full > "$OUT/bench1.log" 2>&1 || { tail -30 "$OUT/bench1.log"; exit 1; }
tail -1 "$OUT/bench1.log"
fi
