# Round 6: the Full replay probe, then the Full bench line (parity checked over all 2582 frames).
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
P=${P:-r6fa}
EAO_PROBE_PASSES=2 timeout -k 10 300 python -u tools/replay_probe.py full > $OUT/${P}_probe_full.log 2>&1 &&
timeout -k 10 600 python -u bench.py --config full --full > $OUT/${P}_bench_full.log 2>&1
