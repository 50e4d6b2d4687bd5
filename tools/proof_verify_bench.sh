#!/bin/sh
# Batched proof verification at k = 128 (tools/proof_verify_bench.py): call
# times against the host loop, then rocprofv3 kernel traces in runs of their own
# for the per-kernel times.  Every GPU step runs under its own time limit and
# the chain stops at the first failure.
#   usage: tools/proof_verify_bench.sh [output directory, default profiles]
set -u
cd "$(dirname "$0")/.." || exit 1
OUT=${1:-profiles}
LOG=$OUT/proof_verify_batch.log
TRACE=$OUT/proof_verify_trace
mkdir -p "$OUT"
trace() {  # kernel stats of one workload: 3 warm-up + 5 timed calls, no host loop
  echo "# rocprofv3 --kernel-trace --stats: proof_verify_bench.py --workload $1 --no-host-loop --repeats 5 (8 calls)" &&
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$TRACE/$1" -o run -- \
    python3 tools/proof_verify_bench.py --workload "$1" --no-host-loop --repeats 5 > "$TRACE.$1.out" 2>&1 &&
  STATS=$(find "$TRACE/$1" -name "*kernel_stats.csv" | head -1) &&
  head -1 "$STATS" && grep "pv_" "$STATS"
}
{
  echo "# tools/proof_verify_bench.py --workload cells" &&
  timeout -k 10 300 python3 tools/proof_verify_bench.py --workload cells &&
  echo "# tools/proof_verify_bench.py --workload rows" &&
  timeout -k 10 300 python3 tools/proof_verify_bench.py --workload rows &&
  trace cells &&
  trace rows
} > "$LOG" 2>&1
rc=$?
cat "$LOG"
exit $rc
