#!/bin/bash
set -e -o pipefail
export OUT=${PNPP_AB_OUT:-ab/mid3}   # where the logs, tables and bench lines go
mkdir -p $OUT
timeout -k 10 400 python -m pytest tests/test_gpu_levels_routed.py tests/test_gpu_split_products.py -x -q -m gpu > $OUT/tests.log 2>&1 || { tail -30 $OUT/tests.log; exit 1; }
tail -3 $OUT/tests.log
for i in 1 2; do
PNPP_MID3=0 PNPP_BENCH_DUMP=$OUT/table_off_$i.txt timeout -k 10 200 python3 bench.py --full --steps 200 --warmup 20 --no-cpu-baseline --no-bf16-variant --no-mfma-variant > $OUT/bench_off_$i.json 2>/dev/null
PNPP_BENCH_DUMP=$OUT/table_on_$i.txt timeout -k 10 200 python3 bench.py --full --steps 200 --warmup 20 --no-cpu-baseline --no-bf16-variant --no-mfma-variant > $OUT/bench_on_$i.json 2>/dev/null
done
grep -h "gemm_mid" $OUT/table_*.txt
python3 - <<'PY'
import json,glob,os
for f in sorted(glob.glob(os.environ["OUT"] + "/bench_*.json")):
    d=json.loads(open(f).read().strip().splitlines()[-1]); print(f, d["value"], d["ms_per_step"])
PY
