#!/bin/sh
# txs -> DAH with the square built on the host against the square written on the
# device (tools/square_device_bench.py), then a rocprofv3 kernel trace of the
# single-block part in a run of its own for the write kernel's own time.  Every
# GPU step runs under its own time limit and the chain stops at the first failure.
#   usage: tools/square_device_bench.sh [output directory, default profiles]
set -u
cd "$(dirname "$0")/.." || exit 1
OUT=${1:-profiles}
LOG=$OUT/square_device.log
TRACE=$OUT/square_device_trace
mkdir -p "$OUT"
{
  echo "# tools/square_device_bench.py" &&
  { timeout -k 10 420 python3 tools/square_device_bench.py 2> "$TRACE.err" || { cat "$TRACE.err"; false; }; } &&
  echo "# rocprofv3 --kernel-trace --stats: square_device_bench.py --skip-batch --repeats 10" &&
  timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$TRACE" -o run -- \
    python3 tools/square_device_bench.py --skip-batch --repeats 10 > "$TRACE.out" 2>&1 &&
  echo "# square_write_kernel, one 128 x 128 square per call, from that trace" &&
  python3 - "$(find "$TRACE" -name "*kernel_trace.csv" | head -1)" <<'PYEOF'
import csv, statistics, sys
v = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in csv.DictReader(open(sys.argv[1]))
     if "square_write" in r["Kernel_Name"]]
print(f"square_write_kernel calls={len(v)} median_us={statistics.median(v) / 1e3:.2f} "
      f"min_us={min(v) / 1e3:.2f} max_us={max(v) / 1e3:.2f}")
PYEOF
} > "$LOG" 2>&1
rc=$?
cat "$LOG"
exit $rc
