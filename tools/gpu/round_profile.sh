# headline bench (--full: with the CPU baseline and kernel-sum probes) + rocprofv3 kernel-trace
# stats of the plain command + PMC traffic passes (separate runs, per MI355X_MICROARCH.md);
# outputs under $OUT (default bench_out/), copied to profiles/ by hand
set -e
export PYTHONUNBUFFERED=1 TMPDIR=/tmp
OUT="${OUT:-bench_out}"
mkdir -p "$OUT"
timeout -k 10 600 python -u bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o bench --output-format csv -- python3 -u bench.py > "$OUT/bench_rocprof.json" 2> "$OUT/bench_rocprof.err"
timeout -s KILL 120 rocprofv3 --pmc FETCH_SIZE -d "$OUT/pmc" -o fetch --output-format csv -- python3 tools/pmc_probe.py > "$OUT/pmc_fetch.log" 2>&1
timeout -s KILL 120 rocprofv3 --pmc WRITE_SIZE -d "$OUT/pmc" -o write --output-format csv -- python3 tools/pmc_probe.py > "$OUT/pmc_write.log" 2>&1
