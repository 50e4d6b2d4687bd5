#!/usr/bin/env python3
"""Batched nmt range-proof production at k = 128, on one resident square.

  export   dagpu_col_nodes_device (inner levels of the 256 column trees, no leaf
           is hashed) against dagpu_row_nodes_device (leaves and inner levels of
           the 256 row trees) on the same square, HIP events
  produce  dagpu_nmt_prove_batch_device for all 65,536 single-cell row samples
           (HIP events around the call and the host wall time of the call),
           against the only other route for the same requests:
           proof.prove_row_ranges on an EDSSubTreeRootCacher (host wall time,
           nodes brought to the host as bytes); then the 131,072 samples of
           both axes, and the row samples with the share gather
  chain    produce + verify on one stream with no host step in between,
           against the verify call alone on the same proofs

Every timed call is warmed up first, and the calls of one comparison take turns
inside each repeat; medians and the spread of `repeats` runs.  Kernel times come
from a rocprofv3 kernel trace of this script in a run of its own:
tools/nmt_prove_bench.sh.
The node bytes of the batched call must equal the host route's.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "celestia-app_amd"))
from celestia_da import da, device, inclusion, proof, synth  # noqa: E402

K = 128
W = 2 * K


def timed(fns, warmup, repeats):
    """Each fn() enqueues on the current stream.  The functions take turns inside
    every repeat, so that a drift of the machine touches all of them alike.
    Returns [(event ms, host wall ms of the call) lists] in the order of fns."""
    ev, host = [[] for _ in fns], [[] for _ in fns]
    for it in range(warmup + repeats):
        for j, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if it >= warmup:
                ev[j].append(a.elapsed_time(b))
                host[j].append((t1 - t0) * 1e3)
    return list(zip(ev, host))


def stats(prefix, v):
    return {prefix + "_median": round(statistics.median(v), 4), prefix + "_min": round(min(v), 4),
            prefix + "_max": round(max(v), 4)}


class Producer:
    """The raw library call with every buffer allocated once."""

    def __init__(self, ctx, an, reqs, shares):
        self.ctx, self.an = ctx, an
        self.req = np.ascontiguousarray(np.asarray(reqs, np.int64))
        self.n = len(self.req)
        dev = an.nodes.device
        m = W.bit_length() - 1
        self.nodes_cap = self.n * m
        self.shares_cap = int((self.req[:, 3] - self.req[:, 2]).sum()) if shares else 0
        self.nodes = torch.empty(self.nodes_cap * 90, dtype=torch.uint8, device=dev)
        self.ns = torch.empty(self.n * 29, dtype=torch.uint8, device=dev)
        self.shares = torch.empty(self.shares_cap * 512, dtype=torch.uint8, device=dev) if shares else None
        self.desc = np.zeros((self.n, 8), np.int64)
        self.ws = torch.empty(ctx._L.dagpu_nmt_prove_workspace_size(self.n), dtype=torch.uint8, device=dev)
        self.total = ctypes.c_size_t(0)

    def __call__(self):
        an = self.an
        self.ctx.check(self.ctx._L.dagpu_nmt_prove_batch_device(
            self.ctx.handle, K, self.n, self.req.ctypes.data, an.eds.data_ptr(), an.nodes.data_ptr(),
            an.col_inner.data_ptr(), self.nodes.data_ptr(), self.nodes_cap, self.ns.data_ptr(),
            self.shares.data_ptr() if self.shares is not None else None, self.shares_cap, self.desc.ctypes.data,
            ctypes.byref(self.total), self.ws.data_ptr(), torch.cuda.current_stream().cuda_stream))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--no-host-route", action="store_true", help="skip proof.prove_row_ranges (kernel-trace runs)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("nmt_prove_bench: no GPU")
    ctx = da.Context(0)
    L = ctx._L
    ods = synth.random_blob_square(K, 4242)
    sq = device.DeviceSquares(K, 1, ctx=ctx)
    sq.load_ods(np.ascontiguousarray(ods).reshape(1, -1))
    sq.extend()
    torch.cuda.synchronize()
    assert int(sq.status[0]) == 0
    eds = sq.eds[0]
    an = inclusion.EDSAxisNodes(K, eds, ctx)
    stream = torch.cuda.current_stream().cuda_stream

    # 1. column export against the row export
    ws = torch.empty(max(L.dagpu_row_nodes_workspace_size(K), L.dagpu_col_nodes_workspace_size(K)),
                     dtype=torch.uint8, device=eds.device)
    (row_ev, _), (col_ev, _) = timed(
        [lambda: ctx.check(L.dagpu_row_nodes_device(ctx.handle, K, eds.data_ptr(), an.nodes.data_ptr(),
                                                    ws.data_ptr(), stream)),
         lambda: ctx.check(L.dagpu_col_nodes_device(ctx.handle, K, an.nodes.data_ptr(), an.col_inner.data_ptr(),
                                                    ws.data_ptr(), stream))], args.warmup, args.repeats)
    print(json.dumps({"measure": "export", "k": K, **stats("row_nodes_ms", row_ev), **stats("col_nodes_ms", col_ev),
                      "col_over_row": round(statistics.median(col_ev) / statistics.median(row_ev), 4),
                      "repeats": args.repeats}), flush=True)

    # 2. the producer against the host route
    rows = [(0, r, c, c + 1) for r in range(W) for c in range(W)]
    both = rows + [(1, c, r, r + 1) for c in range(W) for r in range(W)]
    p_rows, p_both, p_rows_sh = Producer(ctx, an, rows, False), Producer(ctx, an, both, False), \
        Producer(ctx, an, rows, True)
    (ev_r, host_r), (ev_b, host_b), (ev_s, host_s) = timed([p_rows, p_both, p_rows_sh], args.warmup, args.repeats)
    out = {"measure": "produce", "k": K, "row_samples": len(rows), "nodes": int(p_rows.total.value),
           **stats("rows_event_ms", ev_r), **stats("rows_call_wall_ms", host_r),
           "both_axes_samples": len(both), **stats("both_event_ms", ev_b), **stats("both_call_wall_ms", host_b),
           **stats("rows_with_shares_event_ms", ev_s), "repeats": args.repeats,
           "emit_mapping": "one lane per output node (the only mapping built)"}
    if not args.no_host_route:
        cacher = inclusion.EDSSubTreeRootCacher(K, eds, ctx)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_proofs = proof.prove_row_ranges(cacher, [(r, c, c + 1) for _, r, c, _ in rows])
        host_ms = (time.perf_counter() - t0) * 1e3
        got = p_rows.nodes[:90 * p_rows.total.value].cpu().numpy().tobytes()
        same = got == b"".join(b"".join(p.nodes) for p in host_proofs)
        out.update({"host_route_wall_ms": round(host_ms, 1), "nodes_equal_host_route": same,
                    "host_route_over_rows_event": round(host_ms / statistics.median(ev_r), 1),
                    "host_route_over_rows_call_wall": round(host_ms / statistics.median(host_r), 1)})
        assert same, "batched producer and prove_row_ranges disagree"
    out["both_over_rows_event"] = round(statistics.median(ev_b) / statistics.median(ev_r), 3)
    print(json.dumps(out), flush=True)

    # 3. produce + verify on one stream against verify alone
    roots = torch.cat([sq.row_roots[0].reshape(-1), sq.col_roots[0].reshape(-1)])
    p_rows_sh()
    torch.cuda.synchronize()
    desc = p_rows_sh.desc.copy()
    nodes = p_rows_sh.nodes[:90 * p_rows_sh.total.value]
    vws = torch.empty(L.dagpu_nmt_verify_workspace_size(len(desc), int(desc[:, 2].sum())), dtype=torch.uint8,
                      device=eds.device)
    status = []

    def verify():
        status[:] = [device.nmt_verify_batch_device(desc, p_rows_sh.ns, p_rows_sh.shares, 512, nodes, roots, ctx=ctx,
                                                    workspace=vws)]

    def chain():
        p_rows_sh()
        verify()

    (ev_v, _), (ev_c, host_c) = timed([verify, chain], args.warmup, args.repeats)
    ok = int((status[0].cpu().numpy() == 0).sum())
    print(json.dumps({"measure": "chain", "k": K, "proofs": len(desc), **stats("verify_alone_ms", ev_v),
                      **stats("produce_verify_ms", ev_c), **stats("produce_verify_call_wall_ms", host_c),
                      "chain_over_verify": round(statistics.median(ev_c) / statistics.median(ev_v), 3),
                      "verify_alone_ms_recorded_earlier": 0.571, "ok": ok, "repeats": args.repeats}), flush=True)
    assert ok == len(desc)
    ctx.close()


if __name__ == "__main__":
    main()
