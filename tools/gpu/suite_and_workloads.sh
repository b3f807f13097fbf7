# full GPU suite, then the secondary workloads' bench lines (--full: atlas_c4's per-kernel
# figures come from the extra sequential-frame iteration); outputs under $OUT (default bench_out/)
export PYTHONUNBUFFERED=1
set -e
OUT="${OUT:-bench_out}"
mkdir -p "$OUT"
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > "$OUT/gpu_tests.log" 2>&1
timeout -k 10 300 python -u bench.py --workload two_set_50k_exact > "$OUT/bench_c2x.json" 2> "$OUT/bench_c2x.err"
timeout -k 10 300 python -u bench.py --workload two_set_50k > "$OUT/bench_c2.json" 2> "$OUT/bench_c2.err"
timeout -k 10 300 python -u bench.py --workload atlas_c4 --full --no-cpu-baseline > "$OUT/bench_c4.json" 2> "$OUT/bench_c4.err"
