#!/usr/bin/env python3
"""Namespace proofs at k = 128 on one resident square: 1 namespace and 1,024.

The square has 1,024 namespaces in runs of 16 shares (8 per Q0 row).  The
1,024-query list is 960 of them plus 64 ids that fall between two runs (absent
inside a row, or outside every row at a row boundary); the single query is one
present namespace.

  produce  dagpu_nmt_prove_namespace_batch_device (search, layout, emit, share
           gather and leaf hashes, outputs left in HBM; capacities known)
           against the route available without it: D2H of the level-0
           namespaces and the row roots, a numpy search (searchsorted per row),
           dagpu_nmt_prove_batch_device with hand-made ranges and a node gather
           for the absence leaf hashes (outputs left in HBM as well).
  verify   dagpu_nmt_verify_namespace_batch_device on the produced proofs
           (resident) and dagpu_nmt_verify_namespace_batch (host buffers: upload
           included) against a host loop over dagpu_nmt_verify_namespace with
           every buffer already on the host.

Host wall time of each whole step, device synchronised before and after; the
two sides of a comparison take turns inside each repeat.  Both sides must give
the same proofs and every proof must verify.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "celestia-app_amd"))
from celestia_da import da, device, inclusion, synth  # noqa: E402

K = 128
W = 2 * K
RUN = 16


def ns_id(v):
    return b"\x00" * 19 + v.to_bytes(10, "big")


def wall(fns, warmup, repeats):
    out = [[] for _ in fns]
    for it in range(warmup + repeats):
        for j, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= warmup:
                out[j].append((time.perf_counter() - t0) * 1e3)
    return out


def stats(prefix, v):
    return {prefix + "_median": round(statistics.median(v), 4), prefix + "_min": round(min(v), 4),
            prefix + "_max": round(max(v), 4)}


class Today:
    """The route without the namespace calls."""

    def __init__(self, ctx, an, row_roots, queries):
        self.ctx, self.an, self.row_roots = ctx, an, row_roots
        self.q = np.frombuffer(b"".join(queries), dtype="S29")

    def produce(self):
        an = self.an
        lvl0 = an.nodes[:W * W * 96].view(W * W, 96)[:, :29].contiguous().cpu().numpy()
        roots = self.row_roots.cpu().numpy().reshape(W, 90)
        ns = np.frombuffer(lvl0.tobytes(), dtype="S29").reshape(W, W)
        rmin = np.frombuffer(roots[:, :29].tobytes(), dtype="S29")
        rmax = np.frombuffer(roots[:, 29:58].tobytes(), dtype="S29")
        pairs = []
        for r in range(W):
            inside = np.nonzero((self.q >= rmin[r]) & (self.q <= rmax[r]))[0]
            if not len(inside):
                continue
            lo = np.searchsorted(ns[r], self.q[inside], "left")
            hi = np.searchsorted(ns[r], self.q[inside], "right")
            for qi, a, b in zip(inside.tolist(), lo.tolist(), hi.tolist()):
                pairs.append((qi, r, a, b if b > a else a + 1, b == a))
        pairs.sort()
        reqs = [(0, r, a, b) for _, r, a, b, _ in pairs]
        cells = [np.arange(r * W + a, r * W + b) for _, r, a, b, ab in pairs if not ab]
        absent = [(r, 0, a) for _, r, a, _, ab in pairs if ab]
        nodes, _, _, desc = device.nmt_prove_batch_device(an, reqs, ctx=self.ctx)
        shares = None
        if cells:  # the proven shares of the presence proofs: one gather
            idx = torch.from_numpy(np.concatenate(cells)).to(an.nodes.device)
            shares = an.eds.view(W * W, 512).index_select(0, idx).reshape(-1)
        hashes = None
        if absent:
            # the leaf node of (row, a): depth log2(2k), position a
            req = np.array([(r, W.bit_length() - 1, a) for r, _, a in absent], np.uint32)
            d_req = torch.from_numpy(req).to(an.nodes.device)
            hashes = torch.empty(90 * len(absent), dtype=torch.uint8, device=an.nodes.device)
            self.ctx.check(self.ctx._L.dagpu_row_nodes_gather_device(
                self.ctx.handle, K, an.nodes.data_ptr(), len(absent), d_req.data_ptr(), hashes.data_ptr(),
                torch.cuda.current_stream().cuda_stream))
        self.out = (nodes, shares, hashes, desc, pairs)


class Batch:
    def __init__(self, ctx, an, queries):
        self.ctx, self.an, self.queries = ctx, an, queries
        self.caps = None
        dev = an.nodes.device
        self.ws = torch.empty(ctx._L.dagpu_nmt_namespace_workspace_size(K, len(queries)), dtype=torch.uint8, device=dev)

    def produce(self):
        self.out = device.nmt_prove_namespace_batch_device(self.an, self.queries, caps=self.caps, ctx=self.ctx,
                                                           workspace=self.ws)
        c = self.out[6]
        self.caps = (int(c[0]), int(c[2]), int(c[3]), int(c[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("nmt_namespace_bench: no GPU")
    ctx = da.Context(0)
    L = ctx._L
    ods = synth.random_blob_square(K, 4242).copy()
    n_runs = K * K // RUN
    for j in range(n_runs):
        ods[j * RUN:(j + 1) * RUN, :29] = np.frombuffer(ns_id(16 + 2 * j), np.uint8)
    sq = device.DeviceSquares(K, 1, ctx=ctx)
    sq.load_ods(np.ascontiguousarray(ods).reshape(1, -1))
    sq.extend()
    torch.cuda.synchronize()
    assert int(sq.status[0]) == 0
    an = inclusion.EDSAxisNodes(K, sq.eds[0], ctx)
    d_roots = sq.row_roots[0].reshape(-1).contiguous()
    many = [ns_id(16 + 2 * j) for j in range(960)] + [ns_id(17 + 2 * j) for j in range(64)]
    for label, queries in (("1", [ns_id(16 + 2 * 500)]), ("1024", many)):
        today, batch = Today(ctx, an, d_roots, queries), Batch(ctx, an, queries)
        batch.produce()  # learns the capacities, as a server that keeps its buffers would
        t_today, t_batch = wall([today.produce, batch.produce], args.warmup, args.repeats)
        nodes, ns, shares, hashes, desc, pairs, counts = batch.out
        t_nodes, t_shares, t_hashes, t_desc, t_pairs = today.out
        same = (t_nodes.cpu().numpy().tobytes() == nodes.cpu().numpy().tobytes()
                and (t_shares.cpu().numpy().tobytes() if t_shares is not None else b"") == shares.cpu().numpy().tobytes()
                and (t_hashes.cpu().numpy().tobytes() if t_hashes is not None else b"") == hashes.cpu().numpy().tobytes()
                and [(q, r) for q, r, _, _, _ in t_pairs] == [tuple(p) for p in pairs.tolist()])
        print(json.dumps({"measure": "produce", "k": K, "namespaces": label, "proofs": int(counts[0]),
                          "absent": int(counts[1]), "nodes": int(counts[2]), "cells": int(counts[3]),
                          **stats("today_wall_ms", t_today), **stats("batch_wall_ms", t_batch),
                          "today_over_batch": round(statistics.median(t_today) / statistics.median(t_batch), 3),
                          "same_proofs": same, "repeats": args.repeats}), flush=True)
        assert same, "the two routes disagree"

        # verification: everything on the host for the loop and the host-buffer form
        h_nodes, h_shares, h_hashes = (t.cpu().numpy() for t in (nodes, shares, hashes))
        h_ns, h_roots = ns.cpu().numpy(), d_roots.cpu().numpy()
        n = len(desc)
        st_loop = np.zeros(n, np.int32)

        def loop():
            fn = L.dagpu_nmt_verify_namespace
            nb, sb, hb, qb, rb = (x.ctypes.data for x in (h_nodes, h_shares, h_hashes, h_ns, h_roots))
            for i, d in enumerate(desc.tolist()):
                st_loop[i] = fn(qb + 29 * d[6], sb + 512 * d[3], d[2], 512, d[0], d[1], nb + 90 * d[5], d[4],
                                hb + 90 * d[8] if d[8] >= 0 else None, rb + 90 * d[7])

        st_host = np.zeros(n, np.int32)

        def host_form():
            ctx.check(L.dagpu_nmt_verify_namespace_batch(
                ctx.handle, n, desc.ctypes.data, h_ns.ctypes.data, len(queries), h_shares.ctypes.data,
                len(h_shares) // 512, 512, h_nodes.ctypes.data, len(h_nodes) // 90, h_hashes.ctypes.data,
                len(h_hashes) // 90, h_roots.ctypes.data, W, st_host.ctypes.data))

        vws = torch.empty(L.dagpu_nmt_verify_namespace_workspace_size(n, int(desc[:, 2].sum())), dtype=torch.uint8,
                          device=an.nodes.device)
        st_dev = []

        def device_form():
            st_dev[:] = [device.nmt_verify_namespace_batch_device(desc, ns, shares, 512, nodes, hashes, d_roots, ctx=ctx,
                                                                  workspace=vws)]

        t_loop, t_host, t_dev = wall([loop, host_form, device_form], args.warmup, args.repeats)
        ok = (int((st_loop == 0).sum()), int((st_host == 0).sum()), int((st_dev[0].cpu().numpy() == 0).sum()))
        print(json.dumps({"measure": "verify", "k": K, "namespaces": label, "proofs": n,
                          **stats("host_loop_wall_ms", t_loop), **stats("batch_host_buffers_wall_ms", t_host),
                          **stats("batch_device_wall_ms", t_dev),
                          "loop_over_host_buffers": round(statistics.median(t_loop) / statistics.median(t_host), 3),
                          "loop_over_device": round(statistics.median(t_loop) / statistics.median(t_dev), 3),
                          "ok": ok, "repeats": args.repeats}), flush=True)
        assert ok == (n, n, n)
    ctx.close()


if __name__ == "__main__":
    main()
