#!/usr/bin/env python3
"""ProcessProposal's data-parallel part for full blocks (2,000 normal + 2,000
blob txs with real MsgPayForBlobs, the workload of tools/blobtx_validate_bench.py),
raw txs in, one (accept, reason) per block out, by the two routes that exist:

  parent  load_txs(plan="device") (reads the status words), extend(),
          process_proposals(data_hashes): validate_blob_txs reads the planner's
          records, check_commitments downloads the plan arena, lays the tables
          out on the host and uploads them, the verdict is composed in Python
  blocks  process_blocks(blocks, data_hashes): upload, enqueue, one read of
          n x 4 words

for 64 blocks and for one block, the routes taking turns inside every repeat.
Both are bounded by the Python packing of the txs, so two spans are reported:
the whole call, and the time from "upload done" (plan_squares_device has
returned: the packed batch has left host memory) to "verdicts on the host".
Wall times are host clocks around a synchronised device.  Kernel times come
from a rocprofv3 kernel trace in a run of its own (--summarise reads the
trace): the parent's bt_tie and commit_*_kernel beside the counted forms.  Every blob of this workload has at most 7 shares, so all
subtrees have one leaf and nwork = 0: the counted subtree kernel's time in that
trace is its empty-stride cost.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "celestia-app_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("sp_classify", "sp_plan_blocks", "square_write_planned", "bt_validate", "bt_finish", "bt_tie",
           "commit_leaf_kernel", "commit_subtree_kernel", "commit_root_kernel", "cp_reduce", "cp_scan", "cp_fill",
           "bt_tie_counted", "commit_leaf_counted_kernel", "commit_subtree_counted_kernel",
           "commit_root_counted_kernel", "pv_fold", "pv_finish")


def summarise(path):
    rows = list(csv.DictReader(open(path)))
    for name in KERNELS:
        v = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if f"::{name}(" in r["Kernel_Name"]]
        if v:
            print(f"dagpu::{name:<30} launches {len(v):3d}  median {statistics.median(v):9.1f} us  "
                  f"min {min(v):9.1f} us  max {max(v):9.1f} us")


def stats(prefix, v):
    return {prefix + "_median": round(statistics.median(v), 3), prefix + "_min": round(min(v), 3),
            prefix + "_max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--blocks", type=int, nargs="+", default=[64, 1])
    ap.add_argument("--only", choices=("parent", "blocks"))
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    import torch

    from blobtx_validate_bench import full_block_with_pfbs
    from celestia_da import da, device, square as sq
    if not torch.cuda.is_available():
        sys.exit("process_blocks_bench: no GPU")
    ctx = da.Context(0)
    txs = full_block_with_pfbs(ctx)
    k, _ = sq.plan_native(txs)

    # "upload done": the moment plan_squares_device returns to either route
    uploaded = [0.0]
    plan_squares = device.plan_squares_device

    def timed_plan(*a, **kw):
        p = plan_squares(*a, **kw)
        uploaded[0] = time.perf_counter()
        return p
    device.plan_squares_device = timed_plan

    for n in args.blocks:
        blocks = [txs] * n
        d = device.DeviceSquares(k, n, ctx=ctx)
        d.load_txs(blocks, plan="device")
        d.extend()
        torch.cuda.synchronize()
        hashes = [bytes(h) for h in d.dah.cpu().numpy()]

        def parent():
            d.load_txs(blocks, plan="device")
            d.extend()
            return d.process_proposals(data_hashes=hashes)

        def new():
            return d.process_blocks(blocks, data_hashes=hashes)

        routes = [r for r in (("parent", parent), ("blocks", new)) if args.only in (None, r[0])]
        whole = {name: [] for name, _ in routes}
        after = {name: [] for name, _ in routes}
        for it in range(args.warmup + args.repeats):
            for name, run in routes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = run()
                t1 = time.perf_counter()
                assert got == [(True, "")] * n, (name, got[:3])
                if it >= args.warmup:
                    whole[name].append((t1 - t0) * 1e3)
                    after[name].append((t1 - uploaded[0]) * 1e3)
        row = {"measure": "raw txs to verdicts", "k": k, "blocks": n, "txs_per_block": len(txs), "repeats": args.repeats}
        for name, _ in routes:
            row.update(stats(name + "_whole_ms", whole[name]))
            row.update(stats(name + "_after_upload_ms", after[name]))
        if len(routes) == 2:
            row["after_upload_parent_over_blocks"] = round(
                statistics.median(after["parent"]) / statistics.median(after["blocks"]), 2)
            row["whole_parent_over_blocks"] = round(
                statistics.median(whole["parent"]) / statistics.median(whole["blocks"]), 3)
            counts = d.proposal_check.counts.cpu().numpy().tolist()
            row.update({"nblobs": counts[0], "nshares": counts[1], "nsub": counts[2], "nwork": counts[3]})
        print(json.dumps(row), flush=True)
        del d
    ctx.close()


if __name__ == "__main__":
    main()
