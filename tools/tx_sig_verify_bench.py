#!/usr/bin/env python3
"""Tx signature verification of full blocks (2,000 normal + 2,000 blob txs,
every one signed over its SignDoc with one of 8 keys; the shape of
blobtx_validate_bench.py's block) through verify_tx_signatures_device:

  batch     all n blocks resident after process_blocks: wall time up to a
            synchronise, the time after which the call returns, and the span
            between HIP events recorded around it
  one       the same for one block
  beside    process_blocks on the same batch, taking turns with the batch call
            inside every repeat: what the signatures add to it

Every word must be 0 and equal the host executor's on block 0.  There is no
pass threshold: the honest comparison, the reference's Go verifier, cannot be
built here, so the reference side is unmeasured, and the host executor is the
code under test.  Wall times are host clocks around a synchronised device.  The
two kernels' own times come from a rocprofv3 kernel trace in a run of its own
(--skip-process; --summarise reads the trace).
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

CHAIN_ID = "celestia"


def summarise(path):
    rows = list(csv.DictReader(open(path)))
    for name in ("ts_prepare", "ts_verify", "ts_finish"):
        v = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
        if not v:
            continue
        # the trace holds the batch's launches and the one-block ones, told apart by their grids
        grid = [int(r["Grid_Size_X"]) for r in rows if name in r["Kernel_Name"]]
        both = (("batch    ", max(grid)), ("one block", min(grid)))
        for label, keep in both if max(grid) != min(grid) else (("every call", max(grid)),):
            w = [x for x, g in zip(v, grid) if g == keep]
            print(f"dagpu::{name:<12} {label} launches {len(w):3d}  median {statistics.median(w):10.1f} us  "
                  f"min {min(w):10.1f} us  max {max(w):10.1f} us")


def stats(prefix, v):
    return {prefix + "_median": round(statistics.median(v), 4), prefix + "_min": round(min(v), 4),
            prefix + "_max": round(max(v), 4)}


def full_signed_block(ctx):
    """(txs, account numbers): 2,000 signed MsgSend-like txs of about 300 B and
    2,000 signed BlobTxs of one blob of 1 .. 3,000 B around a real MsgPayForBlobs."""
    import numpy as np

    from blobtx_validate_cases import ADDRS
    from celestia_da import blobtx as bt, secp256k1 as ec, shares as sh, trees
    rng = random.Random(7)
    privs = [0x1000003 * (i + 1) ** 5 + 0xC0FFEE for i in range(8)]
    pubs = [ec.pubkey_of(p) for p in privs]
    accts = [rng.randrange(1, 1 << 32) for _ in range(4000)]

    def signed(i, url, value):
        auth = bt.marshal_auth_info(pubs[i % 8], i, fee=rng.randbytes(20))
        doc = bt.sign_doc_bytes(bt.marshal_sdk_tx(url, value, auth_info=auth), CHAIN_ID, accts[i])
        return bt.marshal_sdk_tx(url, value, auth_info=auth, signatures=[ec.sign(privs[i % 8], doc, 0x51ED + i % 16)])

    txs = [signed(i, "/cosmos.bank.v1beta1.MsgSend", rng.randbytes(120)) for i in range(2000)]
    blobs = [sh.Blob.new(sh.new_namespace_v0(rng.randbytes(10)), rng.randbytes(rng.randrange(1, 3001)))
             for _ in range(2000)]
    commitments = trees.create_commitments([(b.namespace(), b.data, 0) for b in blobs], ctx=ctx)
    for i, (b, c) in enumerate(zip(blobs, commitments)):
        pfb = bt.MsgPayForBlobs(signer=ADDRS[i % 3], namespaces=[b.namespace()], blob_sizes=[len(b.data)],
                                share_commitments=[c], share_versions=[0])
        txs.append(bt.marshal_blob_tx(signed(2000 + i, bt.URL_MSG_PAY_FOR_BLOBS, pfb.marshal()), b))
    return txs, np.array(accts, np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--skip-process", action="store_true")
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    import numpy as np
    import torch

    from celestia_da import _abi, da, device, square as sq
    if not torch.cuda.is_available():
        sys.exit("tx_sig_verify_bench: no GPU")
    import tx_sig_cases as cases
    ctx = da.Context(0)
    txs, accts = full_signed_block(ctx)
    n = args.blocks
    k, _ = sq.plan_native(txs)
    blocks = [txs] * n
    d = device.DeviceSquares(k, n, ctx=ctx, in_place=True)
    verdicts = d.process_blocks(blocks)
    one = device.plan_squares_device([txs], ctx=ctx)
    d_all = torch.from_numpy(np.tile(accts, n).view(np.int64).copy()).cuda()
    d_one = torch.from_numpy(accts.view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    m = {name: [] for name in ("process", "batch_wall", "batch_span", "batch_returns", "one_wall", "one_span")}
    for it in range(args.warmup + args.repeats):
        keep = it >= args.warmup
        if not args.skip_process:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            verdicts = d.process_blocks(blocks)
            torch.cuda.synchronize()
            if keep:
                m["process"].append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record()
        tx_status, block_status, signers = d.verify_signatures(CHAIN_ID, d_all)
        t1 = time.perf_counter()
        ev[1].record()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if keep:
            m["batch_wall"].append((t2 - t0) * 1e3)
            m["batch_span"].append(ev[0].elapsed_time(ev[1]))
            m["batch_returns"].append((t1 - t0) * 1e3)
        t0 = time.perf_counter()
        ev[0].record()
        one_status, _, _ = device.verify_tx_signatures_device(one, CHAIN_ID, d_one, ctx=ctx)
        ev[1].record()
        torch.cuda.synchronize()
        if keep:
            m["one_wall"].append((time.perf_counter() - t0) * 1e3)
            m["one_span"].append(ev[0].elapsed_time(ev[1]))
    want = cases.verify_host([txs], accts, chain_id=CHAIN_ID)
    same = (not bool(tx_status.any()) and not bool(one_status.any()) and bool((block_status[:, 0] == -1).all())
            and not want[0].any() and np.array_equal(signers[:len(txs)].cpu().numpy(), want[2]))
    sigs = n * len(txs)
    row = {"measure": "tx signature verification (secp256k1 ECDSA over SHA-256(SignDoc))", "k": k, "blocks": n,
           "txs_per_block": len(txs), "signatures": sigs,
           **stats("batch_wall_ms", m["batch_wall"]), **stats("batch_event_span_ms", m["batch_span"]),
           **stats("batch_call_returns_ms", m["batch_returns"]), **stats("one_block_wall_ms", m["one_wall"]),
           **stats("one_block_event_span_ms", m["one_span"]),
           "ns_per_signature_batch": round(statistics.median(m["batch_span"]) * 1e6 / sigs, 1),
           "ns_per_signature_one_block": round(statistics.median(m["one_span"]) * 1e6 / len(txs), 1),
           "all_words_ok_and_equal_host": same, "all_accepted": all(v[0] for v in verdicts),
           "reference_go_verifier": "unmeasured", "repeats": args.repeats}
    if m["process"]:
        row.update({**stats("process_blocks_wall_ms", m["process"]),
                    "signatures_over_process_blocks": round(statistics.median(m["batch_wall"]) /
                                                            statistics.median(m["process"]), 3)})
    assert same, "a signature word differs from 0 or from the host executor"
    print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
