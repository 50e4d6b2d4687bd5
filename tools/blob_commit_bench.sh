#!/bin/sh
# Share commitments of full 128 x 128 blocks by the host route, the row-node
# store route and the call on resident squares (tools/blob_commit_bench.py),
# for 1 block and for 64, each in a process of its own.  Every GPU step runs
# under its own time limit and the chain stops at the first failure.
#   usage: tools/blob_commit_bench.sh [output directory, default profiles]
set -u
cd "$(dirname "$0")/.." || exit 1
OUT=${1:-profiles}
LOG=$OUT/blob_commit_device.log
mkdir -p "$OUT"
{
  echo "# tools/blob_commit_bench.py --blocks 1" &&
  { timeout -k 10 300 python3 tools/blob_commit_bench.py --blocks 1 2> "$LOG.err" || { cat "$LOG.err"; false; }; } &&
  echo "# tools/blob_commit_bench.py --blocks 64" &&
  { timeout -k 10 420 python3 tools/blob_commit_bench.py --blocks 64 2> "$LOG.err" || { cat "$LOG.err"; false; }; }
} > "$LOG" 2>&1
rc=$?
rm -f "$LOG.err"
cat "$LOG"
exit $rc
