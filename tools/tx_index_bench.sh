#!/bin/sh
# The tx index of 64 resident 128 x 128 blocks against the routes before it
# (tools/tx_index_bench.py), then a rocprofv3 kernel trace of the table routes
# in a run of its own for each kernel's own time and the rate it reaches against
# the bytes it has to move.  Every GPU step runs under its own time limit and
# the chain stops at the first failure.
#   usage: tools/tx_index_bench.sh [output directory, default profiles]
set -u
cd "$(dirname "$0")/.." || exit 1
OUT=${1:-profiles}
LOG=$OUT/tx_index_device.log
TRACE=$OUT/tx_index_trace
mkdir -p "$OUT"
{
  echo "# tools/tx_index_bench.py" &&
  { timeout -k 10 540 python3 tools/tx_index_bench.py 2> "$TRACE.err" || { cat "$TRACE.err"; false; }; } &&
  echo "# rocprofv3 --kernel-trace --stats: tx_index_bench.py --table-only --repeats 5" &&
  timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$TRACE" -o run -- \
    python3 tools/tx_index_bench.py --table-only --repeats 5 > "$TRACE.out" 2>&1 &&
  echo "# kernels of the unit table, 64 squares per call, from that trace" &&
  python3 - "$(find "$TRACE" -name "*kernel_trace.csv" | head -1)" "$TRACE.out" <<'PYEOF'
import collections, csv, json, statistics, sys
t = collections.defaultdict(list)
for r in csv.DictReader(open(sys.argv[1])):
    for name in ("square_units_local", "square_units_carry", "square_units_emit", "square_units_final"):
        if name in r["Kernel_Name"]:
            t[name].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
line = next(json.loads(x) for x in open(sys.argv[2]) if x.startswith("{"))
need = {"square_units_local": line["units_local_bytes"], "square_units_emit": line["units_emit_bytes"]}
for name, v in t.items():
    med = statistics.median(v)
    rate = f" bytes_needed={need[name]} rate_GBps={need[name] / med:.1f}" if name in need else ""
    print(f"{name} calls={len(v)} median_us={med / 1e3:.2f} min_us={min(v) / 1e3:.2f} max_us={max(v) / 1e3:.2f}{rate}")
PYEOF
} > "$LOG" 2>&1
rc=$?
cat "$LOG"
exit $rc
