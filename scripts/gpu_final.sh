#!/bin/bash
# Short GPU-box recipe for a round's last check: GPU tests, smoke, the default bench line and a
# rocprofv3 kernel-trace summary of the bench's engine step.  Outputs under $OUT (default: bench_out/ in the repository).
set -eo pipefail
R=$GRAFT_REPO_ROOT
cd $R
OUT=${OUT:-$R/bench_out}
mkdir -p "$OUT"
timeout -k 10 600 python -u -m pytest -x -q --timeout 120 --timeout-method thread -m gpu tests/ > $OUT/gpu_tests.log 2>&1
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1
timeout -k 10 300 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err
export TMPDIR=/tmp
cd /tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o run -- \
  python3 $R/bench.py --full --steps 100 --no-cpu-baseline --no-configs1 --stream-steps 0 > $OUT/prof.log 2>&1
