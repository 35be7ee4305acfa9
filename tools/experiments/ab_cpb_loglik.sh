#!/bin/bash
# chunks per block on the fused log-likelihood launch of C3 (exact classes): PMX_TUNE_CPB sweep, one box
OUT=${OUT:-runs/ab_cpb_loglik}; mkdir -p $OUT
for rep in 1 2; do for cpb in 0 1 2 3 4 6 8; do
  PMX_TUNE_CPB=$cpb timeout -k 10 200 python bench.py --full --loglik --no-cpu-baseline --steps 20 > $OUT/c.json 2>/dev/null || echo FAIL
  python3 - "$cpb" "$OUT" <<'PY'
import json,sys
d=json.loads(open(sys.argv[2] + "/c.json").read().strip().splitlines()[-1]); r=d["roofline"]
print("cpb", sys.argv[1], "loglik kernel_ms", round(r["kernel_ms"],4), d["parity_ok"])
PY
done; done
