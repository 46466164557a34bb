# Quick state check: EAO bench + association replay probe.
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 400 python -u bench.py --full > $OUT/r4_bench0.log 2>&1 &&
timeout -k 10 200 python -u tools/replay_probe.py > $OUT/r4_probe0.log 2>&1
