#!/bin/bash
# One GPU-box round trip: full GPU test suite, then smoke, then the full bench
# (each step only if the one before it succeeded).  Logs go to the directory
# given as the first argument (default: logs/).
OUT=${1:-logs}
mkdir -p "$OUT"
timeout -k 10 1000 python -m pytest tests -m gpu -q --tb=short -x > "$OUT/pytest_gpu.log" 2>&1
rc=$?
tail -25 "$OUT/pytest_gpu.log" | grep -v -E "^(RCCL|HIP|ROCm|Hostname|Librccl)"
[ $rc -eq 0 ] || exit $rc
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1 &&
timeout -k 10 600 python bench.py --full > "$OUT/bench_default.log" 2>&1
rc=$?
tail -1 "$OUT/bench_default.log"
exit $rc
