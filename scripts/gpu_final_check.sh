# Round-end check: the whole GPU suite and smoke() on the final build, then the bench lines
# (the plain command, and the c3 defaults and c3b with everything reported beside: --full).
set -u
OUT=${OUT:-build/check}
mkdir -p "$OUT/final4"
timeout -k 10 1000 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread \
  > "$OUT/final_gpu_suite.log" 2>&1 || { tail -30 "$OUT/final_gpu_suite.log"; exit 1; }
tail -1 "$OUT/final_gpu_suite.log"
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$OUT/final_smoke.log" 2>&1 \
  || { tail -20 "$OUT/final_smoke.log"; exit 1; }
tail -1 "$OUT/final_smoke.log"
timeout -k 10 400 python bench.py --gpus 1 --steps 20 --warmup 5 > "$OUT/final4/c3_driver.log" 2>&1 || { tail -20 "$OUT/final4/c3_driver.log"; exit 1; }
echo "c3 driver: $(python scripts/bench_line.py "$OUT/final4/c3_driver.log")"
timeout -k 10 400 python bench.py --full > "$OUT/final4/c3_default.log" 2>&1 || { tail -20 "$OUT/final4/c3_default.log"; exit 1; }
echo "c3 default: $(python scripts/bench_line.py "$OUT/final4/c3_default.log")"
timeout -k 10 500 python bench.py --full --config c3b --no-cpu-baseline > "$OUT/final4/c3b.log" 2>&1 || { tail -20 "$OUT/final4/c3b.log"; exit 1; }
echo "c3b: $(python scripts/bench_line.py "$OUT/final4/c3b.log")"
