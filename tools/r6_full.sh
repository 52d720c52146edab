#!/bin/bash
# Round 6: the round-end sequence on one box -- the GPU suite, smoke, the full bench line (and its size):  tools/r6_full.sh OUTDIR
OUT=${1:?usage: tools/r6_full.sh OUTDIR}
mkdir -p "$OUT"
python -m pytest tests -q -m gpu -x --timeout 1200 > "$OUT/gpu_tests.log" 2>&1; echo "pytest rc=$?" >> "$OUT/gpu_tests.log"
tail -4 "$OUT/gpu_tests.log"
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2
python bench.py --full > "$OUT/bench_line.json" 2> "$OUT/bench.err"; echo "bench rc=$?"
wc -c "$OUT/bench_line.json"
cp bench_detail.json "$OUT/bench_detail.json"
OUT="$OUT" python - <<'PY'
import json, os
d = json.loads(open(os.path.join(os.environ["OUT"], "bench_line.json")).read().strip().split("\n")[-1])
print("value", d["value"], "ms", d["ms_per_step"], "frac", d["roofline"]["frac"], "whole", d["roofline"]["whole_step_frac"], "traffic", d["roofline"]["traffic"])
print(json.dumps(d["legs"])[:3000])
PY
