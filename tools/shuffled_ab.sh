#!/bin/bash
# Shuffled C2 A/B: bench --order shuffled per library variant ("cur" = libzkagg.so), 2 rounds interleaved
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-bench_logs}  # where the runs' logs go
mkdir -p "$OUT"
for r in 1 2; do
  for v in "$@"; do
    if [ "$v" = cur ]; then L=$PWD/zipkin_amd/libzkagg.so; else L=$PWD/zipkin_amd/libzkagg_$v.so; fi
    ZKAGG_LIB=$L timeout -k 10 300 python bench.py --order shuffled --steps 10 --cpu-sample 0 > "$OUT/sh_$v.log" 2>&1 || { echo "$v failed"; tail -5 "$OUT/sh_$v.log"; exit 1; }
    python - "$v" "$OUT/sh_$v.log" <<'PY'
import json, sys
j = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
print(sys.argv[1], round(j["ms_per_step"], 3), "ms")
PY
  done
done
