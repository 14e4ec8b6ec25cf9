#!/bin/bash
# Final round-2 validation sweep: full GPU suite + smoke + all benches.
# Logs go to $LOG_DIR (default: validation_logs/, git-ignored).
set -x
LOG_DIR=${LOG_DIR:-validation_logs}
mkdir -p "$LOG_DIR"
timeout 900 python -m pytest tests -m gpu -q 2>&1 | tail -5 | tee "$LOG_DIR/final_pytest.log"
timeout 240 python -c "import __graft_entry__ as ge; ge.smoke(); print('smoke ok')" 2>&1 | tail -3 | tee "$LOG_DIR/final_smoke.log"
timeout 420 python bench.py --full 2>&1 | tail -2 | tee "$LOG_DIR/final_bench.log"
timeout 420 python tools/bench_infer.py 2>&1 | tail -6 | tee "$LOG_DIR/final_infer.log"
timeout 600 python tools/bench_suite.py 3 4 5 2>&1 | tail -4 | tee "$LOG_DIR/final_suite.log"
echo DONE_ALL
