#!/bin/bash
# gemm_wsf03_kernel against gemm_wsf0_kernel on ONE box: the level tests with the new kernel, then the step both ways (PNPP_WSF03=0: the float32-MFMA form)
set -e -o pipefail
export OUT=${PNPP_AB_OUT:-ab/w03}   # where the logs, tables and bench lines go
mkdir -p $OUT
timeout -k 10 500 python -m pytest tests/test_gpu_levels_routed.py tests/test_gpu_split_products.py tests/test_gpu_sa.py -x -q -m gpu > $OUT/tests.log 2>&1 || { tail -40 $OUT/tests.log; exit 1; }
tail -3 $OUT/tests.log
for i in 1 2; do
for v in 0 1; do
PNPP_WSF03=$v PNPP_BENCH_DUMP=$OUT/table_${v}_$i.txt timeout -k 10 200 python3 bench.py --full --steps 200 --warmup 20 --no-cpu-baseline --no-bf16-variant --no-mfma-variant > $OUT/bench_${v}_$i.json 2>/dev/null
done; done
grep -H "gemm_wsf0" $OUT/table_[01]_*.txt
python3 - <<'PY'
import json,glob,os
for f in sorted(glob.glob(os.environ["OUT"] + "/bench_[01]_*.json")):
    d=json.loads(open(f).read().strip().splitlines()[-1]); print(f, d["value"], d["ms_per_step"])
PY
