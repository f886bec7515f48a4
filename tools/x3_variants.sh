#!/bin/bash
# A/B of library variants on ONE box with split products on: tools/x3_variants.sh <variant>...  (abx/lib_<variant>.so; abx/lib_stamps.so for the stamps)
set -o pipefail
LIB=3d-pointcloud-orientation-estimation_amd/pnpp_hip/libpnpp_hip.so
export OUT=${PNPP_AB_OUT:-ab/x3}   # where the logs, tables and bench lines go
mkdir -p $OUT
cp $LIB /tmp/lib_keep.so
export PNPP_SPLIT_PRODUCTS=1
for v in "$@"; do
  cp abx/lib_$v.so $LIB
  PNPP_BENCH_DUMP=$OUT/tab_$v.txt timeout -k 10 200 python3 bench.py --full --steps 100 --warmup 20 --no-cpu-baseline > $OUT/b_$v.json 2> $OUT/b_$v.err || { echo "== $v FAILED"; tail -3 $OUT/b_$v.err; continue; }
  echo "== $v $(python3 -c "import json;d=json.loads(open('$OUT/b_$v.json').readline());print(round(d['value']), d['ms_per_step'])")"
  grep -E "wsd3|wsp3|wsf3|wsx3" $OUT/tab_$v.txt
done
if [ -f abx/lib_stamps.so ]; then
  cp abx/lib_stamps.so $LIB
  timeout -k 10 200 python3 tools/wsd3_stamps.py > $OUT/stamps.txt 2>&1; cat $OUT/stamps.txt
fi
cp /tmp/lib_keep.so $LIB
