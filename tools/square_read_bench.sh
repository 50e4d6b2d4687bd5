#!/bin/sh
# Content back out of 64 resident 128 x 128 blocks by four routes
# (tools/square_read_bench.py), then a rocprofv3 kernel trace of the device
# routes in a run of its own for each kernel's own time and the HBM rate it
# reaches against the bytes it has to move.  Every GPU step runs under its own
# time limit and the chain stops at the first failure.
#   usage: tools/square_read_bench.sh [output directory, default profiles]
set -u
cd "$(dirname "$0")/.." || exit 1
OUT=${1:-profiles}
LOG=$OUT/square_read_device.log
TRACE=$OUT/square_read_trace
mkdir -p "$OUT"
{
  echo "# tools/square_read_bench.py" &&
  { timeout -k 10 420 python3 tools/square_read_bench.py 2> "$TRACE.err" || { cat "$TRACE.err"; false; }; } &&
  echo "# rocprofv3 --kernel-trace --stats: square_read_bench.py --skip-host --repeats 5" &&
  timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$TRACE" -o run -- \
    python3 tools/square_read_bench.py --skip-host --repeats 5 > "$TRACE.out" 2>&1 &&
  echo "# kernels of routes c (all content) and d (one namespace), 64 squares per call, from that trace" &&
  python3 - "$(find "$TRACE" -name "*kernel_trace.csv" | head -1)" "$TRACE.out" <<'PYEOF'
import collections, csv, json, statistics, sys
t = collections.defaultdict(list)
for r in csv.DictReader(open(sys.argv[1])):
    for name in ("square_scan_local", "square_scan_carry", "square_scan_emit", "square_scan_final",
                 "square_select_partial", "square_select_carry", "square_select_emit", "square_gather"):
        if name in r["Kernel_Name"]:
            t[name].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
line = next(json.loads(x) for x in open(sys.argv[2]) if x.startswith("{"))
need = {"square_scan_local": line["scan_local_bytes"], "square_scan_emit": line["scan_emit_bytes"],
        "square_select_partial": line["select_bytes_per_pass"], "square_select_emit": line["select_bytes_per_pass"]}
for name, v in t.items():
    if name == "square_gather":  # routes c and d alternate: the long ones are c's
        v = sorted(v)[len(v) // 2:]
        need[name] = line["gather_c_bytes"]
    med = statistics.median(v)
    rate = f" bytes_needed={need[name]} rate_GBps={need[name] / med:.1f}" if name in need else ""
    print(f"{name} calls={len(v)} median_us={med / 1e3:.2f} min_us={min(v) / 1e3:.2f} max_us={max(v) / 1e3:.2f}{rate}")
PYEOF
} > "$LOG" 2>&1
rc=$?
cat "$LOG"
exit $rc
