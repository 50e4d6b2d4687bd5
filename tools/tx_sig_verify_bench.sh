#!/bin/sh
# The signatures of 64 resident full blocks of 4,000 signed txs, and of one
# block, through dagpu_tx_sig_verify_device, taking turns with process_blocks
# on the same batch (tools/tx_sig_verify_bench.py), then a rocprofv3 kernel
# trace of the signature calls in a run of its own for the kernels' own times.
# Every GPU step runs under its own time limit and the chain stops at the first
# failure.
#   usage: tools/tx_sig_verify_bench.sh [output directory, default profiles]
set -u
cd "$(dirname "$0")/.." || exit 1
OUT=${1:-profiles}
LOG=$OUT/tx_sig_verify_device.log
TRACE=$OUT/tx_sig_verify_trace
mkdir -p "$OUT"
{
  echo "# tools/tx_sig_verify_bench.py --blocks 64 --repeats 5" &&
  { timeout -k 10 420 python3 tools/tx_sig_verify_bench.py --blocks 64 --repeats 5 2> "$TRACE.err" || { cat "$TRACE.err"; false; }; } &&
  echo "# rocprofv3 --kernel-trace --stats: tx_sig_verify_bench.py --blocks 64 --repeats 3 --skip-process" &&
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$TRACE" -o run -- \
    python3 tools/tx_sig_verify_bench.py --blocks 64 --repeats 3 --skip-process > "$TRACE.out" 2>&1 &&
  echo "# kernels of one batch of 64 full blocks (256,000 signatures) from that trace" &&
  python3 tools/tx_sig_verify_bench.py --summarise "$(find "$TRACE" -name "*kernel_trace.csv" | head -1)"
} > "$LOG" 2>&1
rc=$?
rm -f "$TRACE.err"
cat "$LOG"
exit $rc
