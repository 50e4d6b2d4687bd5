#!/usr/bin/env python3
"""Share proofs to the data root from 64 resident k = 128 squares.

  build    dagpu_proof_store_device for all 64 squares (one call, a launch count
           that does not depend on the batch) against the only route before it:
           a loop of 64 x (dagpu_row_nodes_device + dagpu_col_nodes_device) into
           the same layout.  HIP events around the whole, and the wall time up
           to the stream's end.  The two stores must hold the same bytes.
  produce  65,536 single-share proofs to the data root, 1,024 random cells per
           square over both axes, shares included: one
           dagpu_nmt_prove_squares_device call against 64 single-square
           dagpu_nmt_prove_batch_device calls plus proof.proofs_from_byte_slices
           on the host per square (the merkle half).  Wall time up to the
           stream's end; the node bytes must be equal.
  blobs    DeviceSquares.blob_proofs() for every blob of 64 full blocks from
           synth.block_txs (8 distinct blocks, each used 8 times): wall time of
           the produce call with its one download, and of the whole call with
           the ShareProof objects built.  No yardstick: reported on its own.

Every timed call is warmed up first and the calls of one comparison take turns
inside each repeat; medians and the range of `repeats` runs.  The launch count
of one store build comes from a rocprofv3 kernel trace of `--only build` in a
run of its own: tools/share_proof_bench.sh.
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
from celestia_da import da, device, proof, synth  # noqa: E402

K = 128
W = 2 * K
N = 64


def timed(fns, warmup, repeats):
    """Each fn() enqueues on the current stream (it may also wait for it).  The
    functions take turns inside every repeat.  Returns per function (event ms,
    wall ms up to the stream's end)."""
    ev, wall = [[] for _ in fns], [[] for _ in fns]
    for it in range(warmup + repeats):
        for j, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if it >= warmup:
                ev[j].append(a.elapsed_time(b))
                wall[j].append((t1 - t0) * 1e3)
    return list(zip(ev, wall))


def stats(prefix, v):
    return {prefix + "_median": round(statistics.median(v), 4), prefix + "_min": round(min(v), 4),
            prefix + "_max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--only", choices=["build", "produce", "blobs"], action="append",
                    help="run only these measures (kernel-trace runs use --only build)")
    args = ap.parse_args()
    only = set(args.only or ["build", "produce", "blobs"])
    if not torch.cuda.is_available():
        sys.exit("share_proof_bench: no GPU")
    ctx = da.Context(0)
    L = ctx._L
    ds = device.DeviceSquares(K, N, ctx=ctx)
    ds.load_ods(synth.blob_squares(K, 2718, 0, N))
    ds.extend()
    torch.cuda.synchronize()
    assert (ds.status.cpu() == 0).all()
    dev = ds.eds.device
    stream = torch.cuda.current_stream().cuda_stream
    store = ds.proof_store()
    torch.cuda.synchronize()

    # the route of before: the same layout filled square by square
    loop = torch.empty_like(store.store)
    ws = torch.empty(max(L.dagpu_row_nodes_workspace_size(K), L.dagpu_col_nodes_workspace_size(K)),
                     dtype=torch.uint8, device=dev)
    one = W * W * 512

    def build_loop():
        for i in range(N):
            rows = loop.data_ptr() + i * store.row_bytes
            ctx.check(L.dagpu_row_nodes_device(ctx.handle, K, ds.eds.data_ptr() + i * one, rows, ws.data_ptr(), stream))
            ctx.check(L.dagpu_col_nodes_device(ctx.handle, K, rows, loop.data_ptr() + store.col_off +
                                               i * store.col_bytes, ws.data_ptr(), stream))

    sws = torch.empty(L.dagpu_proof_store_workspace_size(K, N), dtype=torch.uint8, device=dev)

    def build_batched():
        ctx.check(L.dagpu_proof_store_device(ctx.handle, K, N, ds.eds.data_ptr(), one, store.store.data_ptr(),
                                             sws.data_ptr(), stream))

    if "build" in only:
        (ev_b, wall_b), (ev_l, wall_l) = timed([build_batched, build_loop], args.warmup, args.repeats)
        rows_same = torch.equal(store.store[:N * store.row_bytes], loop[:N * store.row_bytes])
        cols_same = torch.equal(store.store[store.col_off:store.col_off + N * store.col_bytes],
                                loop[store.col_off:store.col_off + N * store.col_bytes])
        roots_same = torch.equal(store.data_roots(), ds.dah)
        print(json.dumps({"measure": "build", "k": K, "squares": N, "store_bytes": store.store.numel(),
                          **stats("batched_event_ms", ev_b), **stats("batched_wall_ms", wall_b),
                          **stats("loop_event_ms", ev_l), **stats("loop_wall_ms", wall_l),
                          "loop_over_batched_event": round(statistics.median(ev_l) / statistics.median(ev_b), 2),
                          "loop_over_batched_wall": round(statistics.median(wall_l) / statistics.median(wall_b), 2),
                          "launches_per_build_expected": 1 + (W.bit_length() - 1) + (2 * W).bit_length(),
                          "rows_equal": rows_same, "cols_equal": cols_same, "data_roots_equal_extend": roots_same,
                          "repeats": args.repeats}), flush=True)
        assert rows_same and cols_same and roots_same

    if "produce" in only:
        rng = np.random.default_rng(31)
        per = 65536 // N
        req = np.zeros((N * per, 5), np.int64)
        req[:, 0] = np.repeat(np.arange(N), per)
        req[:, 1] = rng.integers(0, 2, len(req))
        req[:, 2] = rng.integers(0, W, len(req))
        req[:, 3] = rng.integers(0, W, len(req))
        req[:, 4] = req[:, 3] + 1
        req = req[rng.permutation(len(req))]
        by_square = [np.ascontiguousarray(req[req[:, 0] == i][:, 1:]) for i in range(N)]
        squares = [store.square(i) for i in range(N)]
        roots = [[r.tobytes() for r in torch.cat([ds.row_roots[i], ds.col_roots[i]]).cpu().numpy()] for i in range(N)]
        kept = {}

        def batched():
            kept["batched"] = device.nmt_prove_squares_device(store, req, ctx=ctx)

        def single():
            kept["single"] = [device.nmt_prove_batch_device(squares[i], by_square[i], eds=squares[i].eds, ctx=ctx)
                              for i in range(N)]
            kept["merkle"] = [proof.proofs_from_byte_slices(roots[i], ctx)[1] for i in range(N)]

        (ev_p, wall_p), (_, wall_s) = timed([batched, single], args.warmup, args.repeats)
        out = kept["batched"]
        # the same nodes, request by request
        nodes = out.nodes.cpu().numpy()
        pos = {i: 0 for i in range(N)}
        ref_nodes = [kept["single"][i][0].cpu().numpy() for i in range(N)]
        ref_desc = [kept["single"][i][3] for i in range(N)]
        aunts = out.aunts.cpu().numpy().reshape(len(req), -1)
        same = True
        for j, r in enumerate(req):
            i = int(r[0])
            d, rd = out.desc[j], ref_desc[i][pos[i]]
            pos[i] += 1
            same &= nodes[90 * d[5]:90 * (d[5] + d[4])].tobytes() == \
                ref_nodes[i][90 * rd[5]:90 * (rd[5] + rd[4])].tobytes()
            if j % 64 == 0:
                same &= aunts[j].tobytes() == b"".join(kept["merkle"][i][int(r[1]) * W + int(r[2])].aunts)
        print(json.dumps({"measure": "produce", "k": K, "squares": N, "proofs": len(req),
                          "proof_nodes": int(out.nodes.numel() // 90),
                          **stats("batched_event_ms", ev_p), **stats("batched_wall_ms", wall_p),
                          **stats("single_square_route_wall_ms", wall_s),
                          "single_over_batched_wall": round(statistics.median(wall_s) / statistics.median(wall_p), 2),
                          "equal_single_square_route": bool(same), "repeats": args.repeats}), flush=True)
        assert same

    if "blobs" in only:
        distinct = [synth.block_txs(2000, 2000, 500 + i) for i in range(8)]
        blocks = [distinct[i % 8] for i in range(N)]
        d = device.DeviceSquares(K, N, ctx=ctx, in_place=True)
        d.load_txs(blocks)
        d.extend()
        torch.cuda.synchronize()
        assert (d.status.cpu() == 0).all()
        rec, _ = d.blob_table()
        ranges = [(int(s), int(a), int(a + c)) for s, a, c in rec]
        bstore = d.proof_store()
        req, _ = device.share_proof_requests(K, N, ranges)
        produce_ms, whole_ms = [], []
        for it in range(args.warmup + args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = device.nmt_prove_squares_device(bstore, req, ctx=ctx)
            host = torch.cat((out.nodes, out.shares, out.axis_roots, out.leaf_hashes, out.aunts)).cpu()
            t1 = time.perf_counter()
            proofs = d.blob_proofs()
            t2 = time.perf_counter()
            if it >= args.warmup:
                produce_ms.append((t1 - t0) * 1e3)
                whole_ms.append((t2 - t1) * 1e3)
            print(f"# blobs repeat {it}: produce+download {(t1 - t0) * 1e3:.1f} ms, blob_proofs() "
                  f"{(t2 - t1) * 1e3:.1f} ms", flush=True)
        sample = list(range(0, len(proofs), max(1, len(proofs) // 256)))
        bad = proof.validate_batch([proofs[i] for i in sample],
                                   [d.dah[int(rec[i, 0])].cpu().numpy().tobytes() for i in sample], ctx)
        print(json.dumps({"measure": "blobs", "k": K, "blocks": N, "blobs": len(ranges), "row_proofs": len(req),
                          "proven_shares": int(rec[:, 2].sum()), "download_bytes": int(host.numel()),
                          **stats("produce_and_download_wall_ms", produce_ms),
                          **stats("blob_proofs_wall_ms", whole_ms),
                          "validated_sample": len(sample), "sample_ok": all(x is None for x in bad),
                          "repeats": args.repeats}), flush=True)
        assert all(x is None for x in bad)
    ctx.close()


if __name__ == "__main__":
    main()
