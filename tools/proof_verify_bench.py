#!/usr/bin/env python3
"""Batched proof verification against the host loop it replaces, at k = 128.

Two workloads from one synthetic square, extended on the device:
  cells  all (2k)^2 = 65,536 single-cell proofs (1 leaf, 8 nodes each); the
         leaves are read from the resident EDS (dagpu_nmt_verify_batch_device
         with d_leaves = the EDS), the nodes from the exported row trees
  rows   256 whole-row proofs (2k leaves, no nodes)

For each: the batch call timed with HIP events around the call (descriptor
check and upload included), warm-up then repeats, median and spread; the host
wall time of the same call; and the only way to do the same work without the
batch entry points: a loop over dagpu_nmt_verify_inclusion on the same bytes in
host memory, in this process.  The statuses of both must agree.

Kernel times (the leaf pass's compressions per second) come from a rocprofv3
kernel trace of this script, taken in a run of its own: tools/proof_verify_bench.sh.
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
from celestia_da import _abi, da, device, inclusion, proof, synth  # noqa: E402

K = 128
W = 2 * K


def build(ctx):
    ods = synth.random_blob_square(K, 4242)
    sq = device.DeviceSquares(K, 1, ctx=ctx)
    sq.load_ods(np.ascontiguousarray(ods).reshape(1, -1))
    sq.extend()
    torch.cuda.synchronize()
    assert int(sq.status[0]) == 0
    cacher = inclusion.EDSSubTreeRootCacher(K, sq.eds[0], ctx)
    # namespace table: every Q0 share's own namespace, then the parity namespace
    ns = np.concatenate([ods[:, :29].reshape(-1), np.full(29, 0xFF, np.uint8)])
    return ods, sq, cacher, torch.from_numpy(ns).to(sq.eds.device)


def cells_workload(ctx, sq, cacher):
    """desc and device nodes of every single-cell proof, row-major."""
    per_col = [proof.range_proof_nodes(W, c, c + 1) for c in range(W)]
    nn = len(per_col[0])
    assert all(len(p) == nn for p in per_col)
    col = np.array(per_col, np.uint32)                       # (W, nn, 2): depth, position
    req = np.empty((W, W, nn, 3), np.uint32)
    req[..., 0] = np.arange(W, dtype=np.uint32)[:, None, None]
    req[..., 1:] = col[None]
    n = W * W
    d_req = torch.from_numpy(req.reshape(-1, 3).view(np.int32)).to(sq.eds.device)
    d_nodes = torch.empty(n * nn * 90, dtype=torch.uint8, device=sq.eds.device)
    ctx.check(ctx._L.dagpu_row_nodes_gather_device(ctx.handle, K, cacher.nodes.data_ptr(), n * nn, d_req.data_ptr(),
                                                   d_nodes.data_ptr(), torch.cuda.current_stream().cuda_stream))
    r, c = np.divmod(np.arange(n, dtype=np.int64), W)
    desc = np.zeros((n, 8), np.int64)
    desc[:, 0], desc[:, 1], desc[:, 2], desc[:, 3] = c, c + 1, 1, np.arange(n)
    desc[:, 4], desc[:, 5] = nn, np.arange(n) * nn
    desc[:, 6] = np.where((r < K) & (c < K), r * K + c, K * K)
    desc[:, 7] = r
    return desc, d_nodes


def rows_workload():
    desc = np.zeros((W, 8), np.int64)
    r = np.arange(W, dtype=np.int64)
    desc[:, 1], desc[:, 2], desc[:, 3] = W, W, r * W
    desc[:, 6] = np.where(r < K, r * K, K * K)   # a Q0 row holds many namespaces: it cannot verify
    desc[:, 7] = r
    return desc, None


def time_batch(ctx, desc, d_ns, d_leaves, d_nodes, d_roots, warmup, repeats):
    n = len(desc)
    dev = d_leaves.device
    if d_nodes is None:
        d_nodes = torch.zeros(96, dtype=torch.uint8, device=dev)
    ws = torch.empty(ctx._L.dagpu_nmt_verify_workspace_size(n, int(desc[:, 2].sum())), dtype=torch.uint8, device=dev)
    ev_ms, host_ms, st = [], [], None
    for it in range(warmup + repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        st = device.nmt_verify_batch_device(desc, d_ns, d_leaves, 512, d_nodes, d_roots, ctx=ctx, workspace=ws)
        b.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        if it >= warmup:
            ev_ms.append(a.elapsed_time(b))
            host_ms.append((t1 - t0) * 1e3)
    return st.cpu().numpy(), ev_ms, host_ms


def host_loop(desc, ns, leaves, nodes, roots):
    f = _abi.lib().dagpu_nmt_verify_inclusion
    a_ns, a_lv, a_nd, a_rt = (x.ctypes.data for x in (ns, leaves, nodes, roots))
    out = np.empty(len(desc), np.int32)
    rows = desc.tolist()
    t0 = time.perf_counter()
    for i, (s, e, nl, lo, nn, no, ni, ri) in enumerate(rows):
        out[i] = f(a_ns + 29 * ni, a_lv + 512 * lo, nl, 512, s, e, a_nd + 90 * no, nn, a_rt + 90 * ri)
    return out, (time.perf_counter() - t0) * 1e3


def report(name, desc, st, ev_ms, host_ms, want, loop_ms):
    n = len(desc)
    leaves = int(desc[:, 2].sum())
    # 9 compressions per 512-B leaf (542-B message), 3 per node hash
    node_hashes = int((desc[:, 4] + desc[:, 2] - 1).sum())
    med = statistics.median(ev_ms)
    print(json.dumps({
        "workload": name, "proofs": n, "leaves": leaves, "node_hashes": node_hashes,
        "compressions": 9 * leaves + 3 * node_hashes,
        "batch_ms_median": round(med, 4), "batch_ms_min": round(min(ev_ms), 4), "batch_ms_max": round(max(ev_ms), 4),
        "batch_host_wall_ms_median": round(statistics.median(host_ms), 4), "repeats": len(ev_ms),
        "host_loop_ms": round(loop_ms, 2), "speedup_vs_host_loop": round(loop_ms / med, 1),
        "ok": int((st == 0).sum()), "statuses_equal_host_loop": bool((st == want).all()),
    }))
    assert (st == want).all(), "batch and host loop disagree"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("cells", "rows", "both"), default="both")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--no-host-loop", action="store_true", help="skip the baseline (kernel-trace runs)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("proof_verify_bench: no GPU")
    ctx = da.Context(0)
    ods, sq, cacher, d_ns = build(ctx)
    eds, roots = sq.eds[0], sq.row_roots[0].reshape(-1)
    h_ns, h_eds, h_roots = d_ns.cpu().numpy(), eds.cpu().numpy(), roots.cpu().numpy()
    for name in ("cells", "rows"):
        if args.workload not in (name, "both"):
            continue
        desc, d_nodes = cells_workload(ctx, sq, cacher) if name == "cells" else rows_workload()
        st, ev_ms, host_ms = time_batch(ctx, desc, d_ns, eds, d_nodes, roots, args.warmup, args.repeats)
        if args.no_host_loop:
            want, loop_ms = st, float("nan")
        else:
            h_nodes = d_nodes.cpu().numpy() if d_nodes is not None else np.zeros(96, np.uint8)
            want, loop_ms = host_loop(desc, h_ns, h_eds, h_nodes, h_roots)
        report(name, desc, st, ev_ms, host_ms, want, loop_ms)
    ctx.close()


if __name__ == "__main__":
    main()
