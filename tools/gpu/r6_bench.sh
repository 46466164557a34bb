# Round 6: the default bench line (EAO) and the Full line, nothing else.
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
P=${P:-r6z}
timeout -k 10 500 python -u bench.py --full > $OUT/${P}_bench.log 2>&1 &&
timeout -k 10 600 python -u bench.py --config full --full > $OUT/${P}_bench_full.log 2>&1
