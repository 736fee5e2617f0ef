#!/bin/bash
# One GPU-box pass: gpu tests, smoke, the whole bench study. Stops at the first failure.
set -o pipefail
O=${OUT:-bench_out}
mkdir -p $O
export PYTHONUNBUFFERED=1
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread -p no:cacheprovider > $O/gpu_tests.log 2>&1 || { echo "gpu tests failed: $?"; tail -40 $O/gpu_tests.log; exit 1; }
tail -5 $O/gpu_tests.log
timeout -k 10 180 python -u -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $O/smoke.log 2>&1 || { echo "smoke failed"; tail -30 $O/smoke.log; exit 1; }
tail -2 $O/smoke.log
timeout -k 10 600 python -u bench.py --full --out $O/bench_detail.json > $O/bench_default.log 2>&1 || { echo "bench failed"; tail -30 $O/bench_default.log; exit 1; }
tail -3 $O/bench_default.log
