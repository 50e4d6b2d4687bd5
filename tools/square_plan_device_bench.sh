#!/bin/sh
# load_txs of full 128 x 128 blocks with the layout made on the host against
# the layout made on the GPU (tools/square_plan_device_bench.py), interleaved in
# one process: 1 block and 256 blocks, alone and followed by extend(); then a
# rocprofv3 kernel trace of device-planned batches in a run of its own, for the
# time of each of the planner's kernels.  Every GPU step runs under its own
# time limit and the chain stops at the first failure.
# Two more builds of the library are used when they are there (both made by
# tools/build_variant.sh, neither is part of the product):
#   celestia-app_amd/libdagpu_parent.so  the parent commit's build: its
#       dagpu_square_plan is timed in turns with this build's
#   celestia-app_amd/libdagpu_clocks.so  this tree with -DDAGPU_PLAN_CLOCKS: the
#       phases of one block's workgroup
#   usage: tools/square_plan_device_bench.sh [output directory, default profiles]
set -u
cd "$(dirname "$0")/.." || exit 1
OUT=${1:-profiles}
LOG=$OUT/square_plan_device.log
PARENT=celestia-app_amd/libdagpu_parent.so
CLOCKS=celestia-app_amd/libdagpu_clocks.so
HOSTLIB=""
[ -f "$PARENT" ] && HOSTLIB="--host-lib $PARENT"
TRACE=$OUT/square_plan_device_trace
mkdir -p "$OUT"
{
  echo "# tools/square_plan_device_bench.py --blocks 256 --repeats 5 $HOSTLIB" &&
  { timeout -k 10 540 python3 tools/square_plan_device_bench.py --blocks 256 --repeats 5 $HOSTLIB 2> "$TRACE.err" ||
    { cat "$TRACE.err"; false; }; } &&
  { [ ! -f "$CLOCKS" ] || {
    echo "# DAGPU_LIB=$CLOCKS tools/square_plan_device_bench.py --phases --blocks 256 --repeats 5" &&
    { DAGPU_LIB=$CLOCKS timeout -k 10 300 python3 tools/square_plan_device_bench.py --phases --blocks 256 --repeats 5 \
        2> "$TRACE.err" || { cat "$TRACE.err"; false; }; }; }; } &&
  echo "# rocprofv3 --kernel-trace --stats: square_plan_device_bench.py --timeline --blocks 256 --repeats 4" &&
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$TRACE" -o run -- \
    python3 tools/square_plan_device_bench.py --timeline --blocks 256 --repeats 4 > "$TRACE.out" 2>&1 &&
  echo "# kernels of one device-planned batch of 256 full blocks: median time over the 4 batches, in launch order" &&
  python3 - "$(find "$TRACE" -name "*kernel_trace.csv" | head -1)" <<'PYEOF'
import collections, csv, statistics, sys
by = collections.OrderedDict()
rows = [r for r in csv.DictReader(open(sys.argv[1]))
        if any(f in r["Kernel_Name"] for f in ("sp_classify", "sp_plan_blocks", "square_write_planned"))]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
for r in rows:
    by.setdefault(r["Kernel_Name"].split("(")[0], []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
for name, v in by.items():
    print(f"{name:40s} launches {len(v):3d}  median {statistics.median(v) / 1e3:10.1f} us")
PYEOF
} > "$LOG" 2>&1
rc=$?
rm -rf "$TRACE" "$TRACE.err" "$TRACE.out"
cat "$LOG"
exit $rc
