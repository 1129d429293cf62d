#!/bin/bash
# Evidence collection on a GPU box, run from the repository root.
# Produces under $OUT (default evidence_out/): bench_*.json, prof_*/
# (rocprofv3 dbs), *_summary.txt (prof_summary tables), pytest_gpu.log
set -x
export TMPDIR=/tmp
OUT=${OUT:-evidence_out}
mkdir -p "$OUT"
python -m pytest tests -m gpu -q 2>&1 | tail -2 | tee "$OUT/pytest_gpu.log"

# bench lines (--full: roofline + cpu_baseline in each)
python bench.py --full --steps 30 --warmup 5 2>/dev/null | tail -1 > "$OUT/bench_bm25_10M.json"
for wl in bm25 range agg; do
  python bench.py --full --workload $wl --docs 100000000 --steps 20 --warmup 3 \
    2>/dev/null | tail -1 > "$OUT/bench_${wl}_100M.json"
done

# kernel-trace profiles of the dominant kernels (no PMC mixed in; plain
# bench runs: the headline path only)
for wl in bm25 agg range; do
  rocprofv3 --kernel-trace --stats -d "$OUT/prof_$wl" -o $wl -- \
    python bench.py --workload $wl --docs 100000000 --steps 5 --warmup 2 \
    > /dev/null 2>&1
  db=$(ls "$OUT"/prof_$wl/*.db 2>/dev/null | head -1)
  [ -n "$db" ] && python tools/prof_summary.py "$db" "$OUT/prof_${wl}_summary.txt"
done

# PMC passes (separate from any tracing): HBM traffic of the agg kernel,
# issue/stall mix of the decode kernel
rocprofv3 --pmc FETCH_SIZE -d "$OUT/pmc_fetch" -o fetch -- \
  python bench.py --workload agg --docs 100000000 --steps 2 --warmup 1 \
  > /dev/null 2>&1
rocprofv3 --pmc WRITE_SIZE -d "$OUT/pmc_write" -o write -- \
  python bench.py --workload agg --docs 100000000 --steps 2 --warmup 1 \
  > /dev/null 2>&1
rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_WAIT_INST_ANY \
  -d "$OUT/pmc_sq" -o sq -- \
  python bench.py --workload bm25 --docs 100000000 --steps 2 --warmup 1 \
  > /dev/null 2>&1
for p in pmc_fetch pmc_write pmc_sq; do
  db=$(ls "$OUT"/$p/*.db 2>/dev/null | head -1)
  [ -n "$db" ] && python tools/prof_summary.py "$db" "$OUT/${p}_summary.txt"
done
rm -rf "$OUT"/prof_*/ "$OUT/pmc_fetch" "$OUT/pmc_write" "$OUT/pmc_sq"
ls -la "$OUT"/
