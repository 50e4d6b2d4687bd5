#!/bin/sh
# Raw txs to verdicts for 64 full blocks and for one, by the parent's route and
# by DeviceSquares.process_blocks (tools/process_blocks_bench.py).  One GPU step
# per invocation, under its own time limit:
#   tools/process_blocks_bench.sh [output directory, default profiles]
#       the two routes interleaved; writes process_blocks_device.log
#   tools/process_blocks_bench.sh [output directory] trace
#       a rocprofv3 kernel trace of both routes, in a run of its own, for the
#       kernels' own times; appends them to the log
set -u
cd "$(dirname "$0")/.." || exit 1
OUT=${1:-profiles}
MODE=${2:-bench}
LOG=$OUT/process_blocks_device.log
TRACE=$OUT/process_blocks_trace
mkdir -p "$OUT"
if [ "$MODE" = trace ]; then
  {
    echo "# rocprofv3 --kernel-trace --stats: process_blocks_bench.py --blocks 64 --repeats 4" &&
    timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d "$TRACE" -o run -- \
      python3 tools/process_blocks_bench.py --blocks 64 --repeats 4 > "$TRACE.out" 2>&1 &&
    echo "# kernels of one batch of 64 full blocks (256,000 txs, 128,000 blobs, nwork = 0) from that trace" &&
    python3 tools/process_blocks_bench.py --summarise "$(find "$TRACE" -name "*kernel_trace.csv" | head -1)"
  } >> "$LOG" 2>&1
  rc=$?
else
  {
    echo "# tools/process_blocks_bench.py --blocks 64 1 --repeats 5" &&
    { timeout -k 10 540 python3 tools/process_blocks_bench.py --blocks 64 1 --repeats 5 2> "$TRACE.err" || { cat "$TRACE.err"; false; }; }
  } > "$LOG" 2>&1
  rc=$?
  rm -f "$TRACE.err"
fi
cat "$LOG"
exit $rc
