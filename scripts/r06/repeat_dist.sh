# The whole bench line (--full) three times in a row (run-to-run spread at the final code), and the
# multi-rank path rehearsed on one GPU: bench.py --gpus 2 over gloo, two ranks sharing the card (a path
# check -- barriers, the accumulator all-reduce, max-over-ranks timing -- not a scaling number).
#   usage: bash scripts/r06/repeat_dist.sh [OUT_DIR]   (default: bench_out/ in the repository root)
cd "$(dirname "$0")/../.." && OUT=${1:-bench_out} && mkdir -p "$OUT/dist" &&
for r in 1 2 3; do
  timeout -k 10 600 python bench.py --full --steps 20 --warmup 5 > "$OUT/rep$r.json" 2> "$OUT/rep$r.err" || exit 1
  python3 -c "import json; d=json.load(open('$OUT/rep$r.json')); print('run $r', d['value'], d['ms_per_step'], {k: t['value'] for k, t in d['targets'].items()}, d['alt_mode']['value'])" | tee -a "$OUT/bench_repeat.txt"
done &&
timeout -k 10 600 python bench.py --gpus 2 --dist-backend gloo --steps 20 --warmup 5 > "$OUT/dist/bench_gloo2_one_gpu.json" 2> "$OUT/dist/bench_gloo2_one_gpu.err" &&
cat "$OUT/dist/bench_gloo2_one_gpu.json"
