OUT=${OUT:-bench_out}; mkdir -p "$OUT"
python bench.py --full --no-cpu-baseline --no-extra-legs > "$OUT/quick.json" 2> "$OUT/quick.err"; python -c "
import json; d=json.load(open('$OUT/quick.json')); print(d['value'], d['ms_per_step']); print({k:(v['ms_per_launch'],v['ms_per_step']) for k,v in d['kernels'].items() if 'pair' in k or 'trimul' in k})"
