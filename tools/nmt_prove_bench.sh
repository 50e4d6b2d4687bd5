#!/bin/sh
# Batched nmt range-proof production at k = 128 (tools/nmt_prove_bench.py): the
# call times against the row export, the host route and the verify call, then a
# rocprofv3 kernel trace in a run of its own for the per-kernel times.  Every GPU
# step runs under its own time limit and the chain stops at the first failure.
#   usage: tools/nmt_prove_bench.sh [output directory, default profiles]
set -u
cd "$(dirname "$0")/.." || exit 1
OUT=${1:-profiles}
LOG=$OUT/nmt_prove_batch.log
TRACE=$OUT/nmt_prove_trace
mkdir -p "$OUT"
{
  echo "# tools/nmt_prove_bench.py" &&
  { timeout -k 10 300 python3 tools/nmt_prove_bench.py 2> "$TRACE.err" || { cat "$TRACE.err"; false; }; } &&
  echo "# rocprofv3 --kernel-trace --stats: nmt_prove_bench.py --no-host-route --repeats 5 (8 calls of each)" &&
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$TRACE" -o run -- \
    python3 tools/nmt_prove_bench.py --no-host-route --repeats 5 > "$TRACE.out" 2>&1 &&
  STATS=$(find "$TRACE" -name "*kernel_stats.csv" | head -1) &&
  head -1 "$STATS" && grep -E "prove_|forest_|pv_" "$STATS" &&
  echo "# median kernel time by grid size (lanes), from the same trace" &&
  python3 - "$(find "$TRACE" -name "*kernel_trace.csv" | head -1)" <<'EOF'
import collections, csv, statistics, sys
by = collections.defaultdict(list)
for r in csv.DictReader(open(sys.argv[1])):
    name = r["Kernel_Name"].split("(")[0]
    if "prove_" in name or "forest_" in name:
        by[(name, int(r["Grid_Size_X"]))].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
for (name, grid), v in sorted(by.items()):
    print(f"{name} lanes={grid} calls={len(v)} median_us={statistics.median(v) / 1e3:.2f} "
          f"min_us={min(v) / 1e3:.2f} max_us={max(v) / 1e3:.2f}")
EOF
} > "$LOG" 2>&1
rc=$?
cat "$LOG"
exit $rc
