#!/bin/bash
# Round 6, first GPU call: the suite + the full bench (is the compact line parseable?) + a timeline of the headline step:  tools/r6_first.sh OUTDIR
OUT=${1:?usage: tools/r6_first.sh OUTDIR}
mkdir -p "$OUT"
python -m pytest tests -q -m gpu -x --timeout 1200 > "$OUT/gpu_tests.log" 2>&1; echo "pytest rc=$?" >> "$OUT/gpu_tests.log"
tail -4 "$OUT/gpu_tests.log"
python bench.py --full --steps 20 --warmup 5 > "$OUT/bench_line.json" 2> "$OUT/bench.err"; echo "bench rc=$?"
wc -c "$OUT/bench_line.json"; cat "$OUT/bench_line.json"
cp bench_detail.json "$OUT/bench_detail_first.json"
TIMELINE=120 tools/prof_cmd.sh "$OUT/step_trace.txt" python bench.py --headline-only --steps 4 --warmup 2 --no-concurrent
head -40 "$OUT/step_trace.txt"
