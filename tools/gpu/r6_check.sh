# Round 6 checkpoint: the GPU suite, smoke, the EAO bench (default run) and the Full bench.
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
P=${P:-r6c}
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread -rs > $OUT/${P}_gputest.log 2>&1 &&
timeout -k 10 150 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/${P}_smoke.log 2>&1 &&
timeout -k 10 500 python -u bench.py --full > $OUT/${P}_bench.log 2>&1 &&
timeout -k 10 600 python -u bench.py --config full --full > $OUT/${P}_bench_full.log 2>&1
