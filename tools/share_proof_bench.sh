#!/bin/sh
# Share proofs to the data root from 64 resident k = 128 squares
# (tools/share_proof_bench.py): the batched store build against the loop of
# single-square exports, the producer across squares against the single-square
# route, every blob's proof of 64 full blocks; then a rocprofv3 kernel trace of
# the store build in a run of its own, for the launch count of one build.  Every
# GPU step runs under its own time limit and the chain stops at the first failure.
#   usage: tools/share_proof_bench.sh [output directory, default profiles]
set -u
cd "$(dirname "$0")/.." || exit 1
OUT=${1:-profiles}
LOG=$OUT/share_proofs_device.log
TRACE=$OUT/share_proofs_trace
mkdir -p "$OUT"
{
  echo "# tools/share_proof_bench.py --only build --only produce" &&
  { timeout -k 10 400 python3 tools/share_proof_bench.py --only build --only produce 2> "$TRACE.err" ||
    { cat "$TRACE.err"; false; }; } &&
  echo "# tools/share_proof_bench.py --only blobs" &&
  { timeout -k 10 600 python3 tools/share_proof_bench.py --only blobs 2> "$TRACE.err" ||
    { cat "$TRACE.err"; false; }; } &&
  echo "# rocprofv3 --kernel-trace --stats: share_proof_bench.py --only build --warmup 1 --repeats 4 (6 batched builds, 5 loops of 64)" &&
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$TRACE" -o run -- \
    python3 tools/share_proof_bench.py --only build --warmup 1 --repeats 4 > "$TRACE.out" 2>&1 &&
  STATS=$(find "$TRACE" -name "*kernel_stats.csv" | head -1) &&
  head -1 "$STATS" && grep -E "store_|forest_" "$STATS" &&
  echo "# launches per build and median kernel time by grid size (lanes), from the same trace" &&
  python3 - "$(find "$TRACE" -name "*kernel_trace.csv" | head -1)" <<'PYEOF'
import collections, csv, statistics, sys
by = collections.defaultdict(list)
store = forest = 0
for r in csv.DictReader(open(sys.argv[1])):
    name = r["Kernel_Name"].split("(")[0]
    if "store_" in name or "forest_" in name:
        by[(name, int(r["Grid_Size_X"]))].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
        store += "store_" in name
        forest += "forest_" in name
print(f"batched build: {store} store_* launches in 6 builds of 64 squares = {store / 6:.1f} per build")
print(f"loop build:    {forest} forest_* launches in 5 loops of 64 squares = {forest / 5:.1f} per loop, "
      f"{forest / 5 / 64:.1f} per square")
for (name, grid), v in sorted(by.items()):
    print(f"{name} lanes={grid} calls={len(v)} median_us={statistics.median(v) / 1e3:.2f} "
          f"min_us={min(v) / 1e3:.2f} max_us={max(v) / 1e3:.2f}")
PYEOF
} > "$LOG" 2>&1
rc=$?
cat "$LOG"
exit $rc
