#!/bin/bash
# the full benchmark line on one GPU: python bench.py --full -> $OUT/bench_$1.json (OUT defaults to bench_out/ in the repository) + a one-line summary
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_out}; mkdir -p "$OUT"
python bench.py --full > "$OUT/bench_$1.json" 2> "$OUT/bench_$1.err"
python - "$OUT/bench_$1.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
r, e = d["roofline"], d["extras"]
print(f"step {d['ms_per_step']} ms = {d['value']} tok/s | GEMM frac {r['frac']} traffic {r['traffic']} probe {r['sustained_mfma_probe']['tflops']} TF | fwd {d['forward_only']['ms_per_step']} | "
      f"cfg2 {e['cfg2']['train_ms_per_step']} / {e['cfg2']['forward_ms']} | cfg5 {e['cfg5']['ms_per_step']} traffic {e['cfg5']['roofline']['traffic']} | cpu {d['cpu_baseline']['value']}")
PY
