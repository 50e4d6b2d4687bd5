#!/usr/bin/env python3
"""Namespace proofs to the data root from 64 resident k = 128 squares: 1
namespace and 1,024.

Every square is a full block of 1,024 namespaces in runs of 16 shares (8 per Q0
row), drawn per square from a universe of 2,048 ids, so a namespace is in about
half of the blocks.  The 1,024-query list is 960 ids of the universe plus 64
ids between two of them (absent inside a row wherever a row's range spans
them); the single query is one namespace of block 0.

  A  the only route before the call across squares: the loop over
     store.square(i) of dagpu_nmt_prove_namespace_batch_device (per square a
     search, a dense read-back, a host layout, an upload, emit; two stream
     synchronisations each; the proofs stop at the row roots)
  B  dagpu_nmt_prove_namespace_squares_device, one call for the batch, with the
     merkle half to the data roots (B) and without it (B0)
  C  dagpu_nmt_namespace_squares_count_device alone, with the per-(query,
     square) counts: "which heights hold my namespaces"

Capacities are known to both routes (taken once, outside the timed region) and
outputs stay in HBM.  Host wall time of each whole route, device synchronised
before and after; the routes take turns inside every repeat.  B must list the
proofs of A, square by square, with the same descriptors everywhere and the
same node, share and leaf-hash bytes in the sampled squares, and every proof of
B must verify, to the row root and on to the data root.  The kernel timeline of
one B call comes from a rocprofv3 kernel trace in a run of its own:
tools/nmt_namespace_squares_bench.sh.
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
from celestia_da import _abi, da, device, synth  # noqa: E402

K = 128
W = 2 * K
N = 64
RUN = 16
UNIVERSE = 2048


def ns_id(v):
    return b"\x00" * 19 + int(v).to_bytes(10, "big")


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


def squares(rng):
    """(N, k*k*512) ODS bytes and per square the sorted universe indexes of its 1,024 runs."""
    ods = synth.blob_squares(K, 2718, 0, N).reshape(N, K * K, 512)
    ids = np.stack([np.frombuffer(ns_id(1000 + 2 * u), np.uint8) for u in range(UNIVERSE)])
    picks = []
    for i in range(N):
        pick = np.sort(rng.choice(UNIVERSE, K * K // RUN, replace=False))
        ods[i, :, :29] = np.repeat(ids[pick], RUN, axis=0)
        picks.append(pick)
    return ods.reshape(N, -1), picks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7, help="alternations of the routes (at least 5)")
    ap.add_argument("--only", choices=["1", "1024"], action="append", help="query counts to run")
    ap.add_argument("--trace", action="store_true", help="only route B with the merkle half (kernel-trace runs)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("nmt_namespace_squares_bench: no GPU")
    if args.repeats < 5 and not args.trace:
        sys.exit("nmt_namespace_squares_bench: at least five alternations")
    rng = np.random.default_rng(41)
    ods, picks = squares(rng)
    ctx = da.Context(0)
    ds = device.DeviceSquares(K, N, ctx=ctx)
    ds.load_ods(ods)
    ds.extend()
    torch.cuda.synchronize()
    assert (ds.status.cpu() == 0).all()
    store = ds.proof_store()
    torch.cuda.synchronize()
    views = [store.square(i) for i in range(N)]
    data_roots = store.data_roots().cpu().numpy().copy()

    drawn = rng.choice(UNIVERSE, 960, replace=False)
    between = rng.choice(UNIVERSE, 64, replace=False)
    many = [ns_id(1000 + 2 * u) for u in drawn] + [ns_id(1001 + 2 * u) for u in between]
    order = rng.permutation(len(many))
    lists = {"1": [ns_id(1000 + 2 * int(picks[0][500]))], "1024": [many[j] for j in order]}

    for name in args.only or ["1", "1024"]:
        qs = lists[name]
        n_q = len(qs)
        caps_a = [device.nmt_namespace_ranges_device(views[i], qs, ctx=ctx)[1][[0, 2, 3, 1]] for i in range(N)]
        counts, per = device.nmt_namespace_squares_count_device(store, qs, ctx=ctx)
        caps_b = counts[[0, 2, 3, 1]]
        kept = {}

        def route_a():
            kept["a"] = [device.nmt_prove_namespace_batch_device(views[i], qs, caps=caps_a[i], ctx=ctx)
                         for i in range(N)]

        def route_b():
            kept["b"] = device.nmt_prove_namespace_squares_device(store, qs, caps=caps_b, ctx=ctx)

        def route_b0():
            kept["b0"] = device.nmt_prove_namespace_squares_device(store, qs, caps=caps_b, to_data_root=False,
                                                                   ctx=ctx)

        def route_c():
            kept["c"] = device.nmt_namespace_squares_count_device(store, qs, ctx=ctx)

        if args.trace:
            wall([route_b], 1, 3)
            continue
        t_a, t_b, t_b0, t_c = wall([route_a, route_b, route_b0, route_c], args.warmup, args.repeats)

        # B lists the proofs of A
        b, a = kept["b"], kept["a"]
        assert np.array_equal(kept["b0"].desc, b.desc) and np.array_equal(kept["c"][0], b.counts)
        assert np.array_equal(kept["c"][1], per) and int(per.sum()) == int(b.counts[0])
        same = int(b.counts[0]) == sum(int(x[6][0]) for x in a)
        sampled = (0, 21, 42, 63)
        host_b = {nm: getattr(b, nm).cpu().numpy() for nm in ("nodes", "shares", "leaf_hashes", "axis_roots")}
        for i in range(N):
            _, _, _, _, desc, pairs, cnt = a[i]
            mine = np.nonzero(b.hits[:, 1] == i)[0]
            same &= len(mine) == len(desc) and np.array_equal(b.hits[mine][:, [0, 2]], pairs)
            same &= np.array_equal(b.desc[mine][:, [0, 1, 2, 4]], desc[:, [0, 1, 2, 4]])
            same &= np.array_equal(b.desc[mine, 8] >= 0, desc[:, 8] >= 0)
            same &= np.array_equal(per[:, i], np.bincount(pairs[:, 0], minlength=n_q))
            if i in sampled:
                an, ash, alh = (a[i][j].cpu().numpy() for j in (0, 2, 3))
                roots = ds.row_roots[i].cpu().numpy()
                for j, d in zip(mine.tolist(), desc.tolist()):
                    e = b.desc[j]
                    same &= host_b["nodes"][90 * e[5]:90 * (e[5] + e[4])].tobytes() == \
                        an[90 * d[5]:90 * (d[5] + d[4])].tobytes()
                    same &= host_b["shares"][512 * e[3]:512 * (e[3] + e[2])].tobytes() == \
                        ash[512 * d[3]:512 * (d[3] + d[2])].tobytes()
                    if d[8] >= 0:
                        same &= host_b["leaf_hashes"][90 * e[8]:90 * e[8] + 90].tobytes() == \
                            alh[90 * d[8]:90 * d[8] + 90].tobytes()
                    same &= host_b["axis_roots"][90 * j:90 * j + 90].tobytes() == roots[d[7]].tobytes()
        # and every proof of B verifies, to the row root and on to the data root
        st = device.nmt_verify_namespace_batch_device(b.desc, b.namespaces, b.shares, 512, b.nodes, b.leaf_hashes,
                                                      b.axis_roots, ctx=ctx).cpu().numpy()
        n = len(b.desc)
        mst = np.full(n, 77, np.int32)
        lv, lh, au = (np.ascontiguousarray(t.cpu().numpy()) for t in (b.axis_roots, b.dah_leaf_hashes, b.aunts))
        md = np.ascontiguousarray(b.mdesc)
        ctx.check(ctx._L.dagpu_merkle_verify_batch(ctx.handle, n, md.ctypes.data, lv.ctypes.data, n, 90,
                                                   lh.ctypes.data, au.ctypes.data, len(au) // 32,
                                                   data_roots.ctypes.data, N, mst.ctypes.data))
        verified = bool((st == _abi.OK).all()) and bool((mst == _abi.OK).all())
        med = {r: statistics.median(v) for r, v in (("a", t_a), ("b", t_b), ("b0", t_b0))}
        print(json.dumps({
            "measure": "namespace_squares", "k": K, "squares": N, "queries": n_q, "lanes": n_q * N * W,
            "proofs": int(b.counts[0]), "absence_proofs": int(b.counts[1]), "proof_nodes": int(b.counts[2]),
            "proven_cells": int(b.counts[3]), "squares_with_a_hit": int((per.sum(axis=0) > 0).sum()),
            **stats("A_loop_wall_ms", t_a), **stats("B_squares_wall_ms", t_b),
            **stats("B0_no_merkle_wall_ms", t_b0), **stats("C_count_wall_ms", t_c),
            "A_over_B": round(med["a"] / med["b"], 2), "A_over_B0": round(med["a"] / med["b0"], 2),
            "ranges_overlap_A_B": not (min(t_a) > max(t_b) or min(t_b) > max(t_a)),
            "equal_single_square_route": bool(same), "sampled_squares": list(sampled), "all_verify": verified,
            "repeats": args.repeats}), flush=True)
        assert same and verified
    ctx.close()


if __name__ == "__main__":
    main()
