#!/bin/sh
# The declared-commitment table of 64 resident full blocks by the host's Python
# walk and by dagpu_blob_tx_validate_device (tools/blobtx_validate_bench.py),
# then a rocprofv3 kernel trace of the device route in a run of its own for the
# kernels' own times.  Every GPU step runs under its own time limit and the
# chain stops at the first failure.
#   usage: tools/blobtx_validate_bench.sh [output directory, default profiles]
set -u
cd "$(dirname "$0")/.." || exit 1
OUT=${1:-profiles}
LOG=$OUT/blobtx_validate_device.log
TRACE=$OUT/blobtx_validate_trace
mkdir -p "$OUT"
{
  echo "# tools/blobtx_validate_bench.py --blocks 64 --repeats 10" &&
  { timeout -k 10 420 python3 tools/blobtx_validate_bench.py --blocks 64 --repeats 10 2> "$TRACE.err" || { cat "$TRACE.err"; false; }; } &&
  echo "# rocprofv3 --kernel-trace --stats: blobtx_validate_bench.py --blocks 64 --repeats 6 --skip-host" &&
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$TRACE" -o run -- \
    python3 tools/blobtx_validate_bench.py --blocks 64 --repeats 6 --skip-host > "$TRACE.out" 2>&1 &&
  echo "# kernels of one batch of 64 full blocks (256,000 txs, 128,000 blobs) from that trace" &&
  python3 tools/blobtx_validate_bench.py --summarise "$(find "$TRACE" -name "*kernel_trace.csv" | head -1)"
} > "$LOG" 2>&1
rc=$?
rm -f "$TRACE.err"
cat "$LOG"
exit $rc
