set -o pipefail
cd "$(dirname "$0")/.."
O=${BENCH_OUT:-out/wu}  # --full: the extras' warm-up is part of the comparison
mkdir -p $O
timeout -k 10 300 python bench.py --full --no-scaling-sim --no-cpu-baseline > $O/a.json 2>/dev/null || exit 1
timeout -k 10 300 python bench.py --full --no-scaling-sim --no-cpu-baseline --warmup 300 --extras-warmup 300 > $O/b.json 2>/dev/null || exit 1
timeout -k 10 300 python bench.py --full --no-scaling-sim --no-cpu-baseline > $O/c.json 2>/dev/null || exit 1
