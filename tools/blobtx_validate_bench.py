#!/usr/bin/env python3
"""The declared-commitment table and the stateless ValidateBlobTx rules of
full blocks (2,000 normal + 2,000 blob txs with real MsgPayForBlobs, the shape
of full_block() of tests/square_corpus.py), resident in HBM after
load_txs(plan="device"), by the two routes that exist:

  host    square.expected_commitments of ONE block: the Python walk of every
          BlobTx and its MsgPayForBlobs, which applies three of the rules; a
          batch of n blocks costs n times this
  device  DeviceSquares.validate_blob_txs over ALL n blocks: every rule, the
          per-tx and per-block words and the table; wall time up to a
          synchronise, the time after which the call returns, and the span
          between HIP events recorded around it (the stream idles inside that
          span while the host fills and uploads its tables, so it is an upper
          bound of the three kernels' time)

The routes take turns inside every repeat and must give the same table.  Wall
times are host clocks around a synchronised device.  Kernel times come from a
rocprofv3 kernel trace in a run of its own (--skip-host; --summarise reads the
trace).
"""
import argparse
import csv
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "celestia-app_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def summarise(path):
    rows = list(csv.DictReader(open(path)))
    for name in ("bt_validate", "bt_finish", "bt_tie", "sp_classify", "sp_plan_blocks"):
        v = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
        if v:
            print(f"dagpu::{name:<16} launches {len(v):3d}  median {statistics.median(v):9.1f} us  "
                  f"min {min(v):9.1f} us  max {max(v):9.1f} us")


def stats(prefix, v):
    return {prefix + "_median": round(statistics.median(v), 4), prefix + "_min": round(min(v), 4),
            prefix + "_max": round(max(v), 4)}


def full_block_with_pfbs(ctx):
    """2,000 normal txs of 300 B and 2,000 BlobTxs of one blob of 1 .. 3,000 B
    around a real MsgPayForBlobs; the commitments from one create_commitments call."""
    from blobtx_validate_cases import ADDRS
    from celestia_da import blobtx as bt, shares as sh, trees
    rng = random.Random(7)
    txs = [rng.randbytes(300) for _ in range(2000)]
    blobs = [sh.Blob.new(sh.new_namespace_v0(rng.randbytes(10)), rng.randbytes(rng.randrange(1, 3001)))
             for _ in range(2000)]
    commitments = trees.create_commitments([(b.namespace(), b.data, 0) for b in blobs], ctx=ctx)
    for i, (b, c) in enumerate(zip(blobs, commitments)):
        pfb = bt.MsgPayForBlobs(signer=ADDRS[i % 3], namespaces=[b.namespace()], blob_sizes=[len(b.data)],
                                share_commitments=[c], share_versions=[0])
        inner = bt.marshal_sdk_tx(bt.URL_MSG_PAY_FOR_BLOBS, pfb.marshal(), auth_info=rng.randbytes(80),
                                  signatures=[rng.randbytes(64)])
        txs.append(bt.marshal_blob_tx(inner, b))
    return txs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    import torch

    from celestia_da import da, device, square as sq
    if not torch.cuda.is_available():
        sys.exit("blobtx_validate_bench: no GPU")
    ctx = da.Context(0)
    txs = full_block_with_pfbs(ctx)
    n = args.blocks
    k, plan = sq.plan_native(txs)
    d = device.DeviceSquares(k, n, ctx=ctx, in_place=True)
    d.load_txs([txs] * n, plan="device")
    torch.cuda.synchronize()
    table = sq.expected_commitments(txs, plan)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    host, wall, span, returns = [], [], [], []
    for it in range(args.warmup + args.repeats):
        torch.cuda.synchronize()
        if not args.skip_host:
            t0 = time.perf_counter()
            sq.expected_commitments(txs, plan)
            h = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record()
        tx_status, block_status, expected = d.validate_blob_txs()
        t1 = time.perf_counter()
        ev[1].record()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if it >= args.warmup:
            if not args.skip_host:
                host.append(h)
            wall.append((t2 - t0) * 1e3)
            span.append(ev[0].elapsed_time(ev[1]))
            returns.append((t1 - t0) * 1e3)
    want = torch.from_numpy(table).cuda()
    same = bool((expected.view(n, len(table), 32) == want).all()) and not bool(tx_status.any()) \
        and bool((block_status[:, 0] == -1).all())
    _, _, sq_status = d.check_commitments(expected="declared")
    row = {"measure": "declared commitments + ValidateBlobTx rules", "k": k, "blocks": n, "txs_per_block": len(txs),
           "blob_txs_per_block": len(table),
           **stats("device_all_blocks_wall_ms", wall), **stats("device_event_span_ms", span),
           **stats("device_call_returns_ms", returns), "tables_equal": same,
           "commitments_match_declared": not bool(sq_status.cpu().any()), "repeats": args.repeats}
    if host:
        row.update({**stats("host_one_block_ms", host),
                    "host_all_blocks_ms_extrapolated": round(statistics.median(host) * n, 1),
                    "host_over_device_wall": round(statistics.median(host) * n / statistics.median(wall), 1)})
    assert same, "the device table differs from square.expected_commitments"
    print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
