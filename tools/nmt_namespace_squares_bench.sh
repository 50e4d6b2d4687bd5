#!/bin/sh
# Namespace proofs to the data root from 64 resident k = 128 squares
# (tools/nmt_namespace_squares_bench.py): the loop of single-square calls
# against the call across squares, for 1 namespace and for 1,024; then a
# rocprofv3 kernel trace of the call across squares at 1,024 namespaces in a run
# of its own, for its launch count and kernel timeline.  Every GPU step runs
# under its own time limit and the chain stops at the first failure.
#   usage: tools/nmt_namespace_squares_bench.sh [output directory, default profiles]
set -u
cd "$(dirname "$0")/.." || exit 1
OUT=${1:-profiles}
LOG=$OUT/nmt_namespace_squares_device.log
TRACE=$OUT/nmt_namespace_squares_trace
mkdir -p "$OUT"
{
  echo "# tools/nmt_namespace_squares_bench.py" &&
  { timeout -k 10 420 python3 tools/nmt_namespace_squares_bench.py 2> "$TRACE.err" ||
    { cat "$TRACE.err"; false; }; } &&
  echo "# rocprofv3 --kernel-trace --stats: nmt_namespace_squares_bench.py --trace --only 1024 (4 calls across squares)" &&
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$TRACE" -o run -- \
    python3 tools/nmt_namespace_squares_bench.py --trace --only 1024 > "$TRACE.out" 2>&1 &&
  echo "# kernels of one call across squares, in launch order: median time over the 4 calls" &&
  python3 - "$(find "$TRACE" -name "*kernel_trace.csv" | head -1)" <<'PYEOF'
import collections, csv, statistics, sys
rows = [r for r in csv.DictReader(open(sys.argv[1]))
        if any(f in r["Kernel_Name"] for f in ("ns_sq_", "ns_leaf_nodes", "prove_"))]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
# the count call that sizes the capacities runs once before the four timed calls: skip its five kernels
finds = [i for i, r in enumerate(rows) if "ns_sq_find" in r["Kernel_Name"]]
calls = [rows[a:b] for a, b in zip(finds, finds[1:] + [len(rows)])][1:]
assert len(calls) == 4 and len({len(c) for c in calls}) == 1, [len(c) for c in calls]
print(f"launches per call: {len(calls[0])}")
total = []
for j in range(len(calls[0])):
    name = calls[0][j]["Kernel_Name"].split("(")[0]
    us = [(int(c[j]["End_Timestamp"]) - int(c[j]["Start_Timestamp"])) / 1e3 for c in calls]
    gap = [(int(c[j]["Start_Timestamp"]) - int(c[j - 1]["End_Timestamp"])) / 1e3 for c in calls] if j else [0.0]
    print(f"{name} grid={calls[0][j]['Grid_Size_X']} median_us={statistics.median(us):.2f} "
          f"min_us={min(us):.2f} max_us={max(us):.2f} gap_before_median_us={statistics.median(gap):.2f}")
    total.append(statistics.median(us))
span = [(int(c[-1]["End_Timestamp"]) - int(c[0]["Start_Timestamp"])) / 1e3 for c in calls]
print(f"kernel time per call: {sum(total):.2f} us; first kernel start to last kernel end, median: "
      f"{statistics.median(span):.2f} us")
PYEOF
} > "$LOG" 2>&1
rc=$?
cat "$LOG"
exit $rc
