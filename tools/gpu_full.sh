#!/bin/bash
# One GPU session: full -m gpu suite, the three bench workloads, a kernel-trace profile of the
# default bench. Every GPU step has its own time limit; a crash / timeout ends the session.
TAG=${1:-full}
R="$(cd "$(dirname "$0")/.." && pwd)"; cd "$R" || exit 1
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
ok() { local rc=$1; [ $rc -eq 0 ] || [ $rc -eq 1 ]; }
timeout -k 10 600 python -u -m pytest tests -m gpu -v --timeout 120 --timeout-method thread \
  > $OUT/${TAG}_pytest.log 2>&1; rc=$?
echo "pytest rc=$rc: $(tail -1 $OUT/${TAG}_pytest.log)"
ok $rc || exit $rc
timeout -k 10 300 python bench.py --full > $OUT/${TAG}_bench_dense.log 2>&1 || exit $?
echo "dense: $(tail -1 $OUT/${TAG}_bench_dense.log | cut -c1-400)"
timeout -k 10 300 python bench.py --full --workload hybrid --steps 20 --warmup 3 \
  > $OUT/${TAG}_bench_hybrid.log 2>&1 || exit $?
echo "hybrid: $(tail -1 $OUT/${TAG}_bench_hybrid.log | cut -c1-300)"
timeout -k 10 400 python bench.py --full --workload hybrid_rerank --steps 5 --warmup 2 --latency-iters 3 \
  > $OUT/${TAG}_bench_rerank.log 2>&1 || exit $?
echo "rerank: $(tail -1 $OUT/${TAG}_bench_rerank.log | cut -c1-300)"
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv \
  -d "$R/$OUT/prof_${TAG}_dense" -o run -- \
  python3 "$R/bench.py" --steps 20 --warmup 3 --no-cpu-baseline --latency-iters 3 \
  > "$R/$OUT/${TAG}_prof_dense.log" 2>&1; rc=$?
echo "prof dense rc=$rc"
[ $rc -eq 0 ] || exit $rc
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv \
  -d "$R/$OUT/prof_${TAG}_rerank" -o run -- \
  python3 "$R/bench.py" --workload hybrid_rerank --steps 3 --warmup 1 --latency-iters 1 \
  > "$R/$OUT/${TAG}_prof_rerank.log" 2>&1; rc=$?
echo "prof rerank rc=$rc"
exit $rc
