#!/bin/bash
# GPU box: bench the hx path for several batch-slice sizes of the triangle multiplication.
cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
for sb in "$@"; do
  GENIE_HX_SLICE=$sb timeout -k 10 200 python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline > "$OUT/slice$sb.json" 2> "$OUT/slice$sb.err" || echo "slice $sb failed"
  python - <<PY
import json
d = json.load(open('$OUT/slice$sb.json'))
print('slice $sb', round(d['value'], 2), {k: round(v['ms_per_step'], 3) for k, v in d['kernels'].items() if v['ms_per_step'] > 0.5})
PY
done
