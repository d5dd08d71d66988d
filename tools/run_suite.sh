#!/bin/bash
# full -m gpu suite + the full bench line (bench.py --full) in one go; logs under $OUT (default logs/), tag = $1
set -o pipefail
tag=${1:-r03}
OUT=${OUT:-logs}
mkdir -p "$OUT"
python -m pytest tests -x -q -m gpu > "$OUT/${tag}_gpu_tests.log" 2>&1
rc=$?
tail -3 "$OUT/${tag}_gpu_tests.log"
[ $rc -ne 0 ] && exit $rc
python bench.py --full > "$OUT/${tag}_bench.json.log" 2> "$OUT/${tag}_bench.err"
rc=$?
tail -c 2500 "$OUT/${tag}_bench.json.log"
exit $rc
