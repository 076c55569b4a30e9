# The cfg4 (Brakedown) bench line with its roofline and oracle checks, then a rocprofv3 kernel trace
# of a shorter run.  Usage (repo root, on a GPU host): bash tools/bench_sdig.sh <output dir>
set -o pipefail
export TMPDIR=/tmp
OUT=${1:?usage: bash tools/bench_sdig.sh <output dir>}
mkdir -p "$OUT"
timeout -k 10 600 python bench.py --full --code sdig --steps 32 --warmup 12 > "$OUT/bench.json" 2> "$OUT/bench.err" || { tail -30 "$OUT/bench.err"; exit 1; }
cat "$OUT/bench.json"
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run --output-format csv -- python3 bench.py --full --code sdig --steps 8 --warmup 4 --cpu-baseline off > /dev/null 2> "$OUT/prof.err" || { tail -30 "$OUT/prof.err"; exit 1; }
