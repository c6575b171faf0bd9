#!/bin/bash
# Round-end evidence run on the MI355X box: full GPU test suite, the bench line (--full), and the rocprofv3 kernel statistics
# of the same bench command. Outputs under the folder OUT names (copy the summaries to profiles/).
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
R=$PWD
OUT=$(mkdir -p "${OUT:?set OUT to the folder for the outputs}" && cd "$OUT" && pwd) || exit 1
export TMPDIR=/tmp
timeout -k 10 900 python -m pytest tests -q -m gpu -x > "$OUT/gpu_tests.log" 2>&1 || { tail -n 30 "$OUT/gpu_tests.log"; exit 1; }
tail -n 3 "$OUT/gpu_tests.log"
timeout -k 10 600 python bench.py --full --steps 10 --warmup 2 > "$OUT/bench_n1.json" 2> "$OUT/bench_n1.err" || { tail "$OUT/bench_n1.err"; exit 1; }
cat "$OUT/bench_n1.json"
(cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -o smm32 -- python3 "$R/bench.py" --full --steps 10 --warmup 2 --no-cpu --no-variants > "$OUT/prof_bench.json" 2> "$OUT/prof_bench.err") || { tail "$OUT/prof_bench.err"; exit 1; }
ls "$OUT/prof"
