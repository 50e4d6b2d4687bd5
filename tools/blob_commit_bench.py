#!/usr/bin/env python3
"""Share commitments of every blob of full 128 x 128 blocks (full_block() of
tests/square_corpus.py: 2,000 normal + 2,000 blob txs), for 1 block and for 64
(the same block 64 times), by the routes that exist:

  a  dagpu_blob_commitments fed the same blobs' shares from host memory (the
     shares cut out of the host-constructed ODS before the clock starts): the
     call repacks, uploads, runs the generic forest and synchronises
  b  inclusion.get_commitment for every blob from the row-node store of the
     extended square (one block only): the store's construction and the loop
  c  dagpu_blob_commitments_device on the squares load_txs wrote in HBM, with
     the declared commitments compared on the device; wall time of the call up
     to a synchronise, the time after which the call returns, and the span
     between HIP events recorded before and after the call (the stream idles
     inside that span while the host builds and uploads the tables, so it is
     an upper bound of the three kernels' time)
  d  txs -> DAH (load_txs, extend, DAH to the host) without and with c enqueued
     on the same stream between the write and the extend

The routes take turns inside every repeat.  a, b and c must give the same
commitments.  Wall times are host clocks around a synchronised device.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from celestia_da import _abi, da, device, inclusion as inc, square as sq  # noqa: E402
from square_corpus import full_block  # noqa: E402

K = 128


def stats(prefix, v):
    return {prefix + "_median": round(statistics.median(v), 4), prefix + "_min": round(min(v), 4),
            prefix + "_max": round(max(v), 4)}


class Bench:
    def __init__(self, ctx, txs, n):
        self.ctx, self.L, self.n, self.txs = ctx, ctx._L, n, txs
        k, ods = sq.construct_native(txs)
        assert k == K
        self.d = device.DeviceSquares(K, n, ctx=ctx, in_place=True)
        self.d.load_txs([txs] * n)
        self.recs, _ = self.d.blob_table()
        self.nb = len(self.recs)
        shares = ods.reshape(K * K, 512)
        one = self.recs[self.recs[:, 0] == 0]
        # route a's input: namespaces, share counts and the shares themselves, packed
        self.a_ns = np.ascontiguousarray(np.tile(np.stack([shares[f, :29] for _, f, _ in one]), (n, 1)))
        self.a_cnt = np.ascontiguousarray(np.tile(one[:, 2].astype(np.uint32), n))
        self.a_shares = np.ascontiguousarray(np.tile(np.concatenate([shares[f:f + c] for _, f, c in one]), (n, 1)))
        self.a_out = np.zeros((self.nb, 32), np.uint8)
        self.nshares = int(self.recs[:, 2].sum())
        # route c's buffers, allocated once
        self.ws = torch.empty((self.L.dagpu_blob_commitments_workspace_size(K, self.nb, self.nshares),),
                              dtype=torch.uint8, device="cuda")
        self.c_out = torch.empty((self.nb, 32), dtype=torch.uint8, device="cuda")
        self.c_st = torch.empty((self.nb,), dtype=torch.int32, device="cuda")
        self.c_sq = torch.empty((n,), dtype=torch.int32, device="cuda")
        self.ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        self.route_a()
        self.expected = torch.from_numpy(self.a_out.copy()).cuda()

    def route_a(self):
        t0 = time.perf_counter()
        self.ctx.check(self.L.dagpu_blob_commitments(self.ctx.handle, self.nb, _abi.addr(self.a_ns),
                                                     _abi.addr(self.a_cnt), _abi.addr(self.a_shares), 64,
                                                     _abi.addr(self.a_out)))
        return (time.perf_counter() - t0) * 1e3

    def enqueue_c(self):
        w = 2 * K
        self.ctx.check(self.L.dagpu_blob_commitments_device(
            self.ctx.handle, K, self.n, self.nb, _abi.addr(self.recs), self.d.eds.data_ptr(), w * w * 512, w * 512,
            64, self.c_out.data_ptr(), self.expected.data_ptr(), self.c_st.data_ptr(), self.c_sq.data_ptr(),
            self.ws.data_ptr(), torch.cuda.current_stream().cuda_stream))

    def route_c(self):
        """-> (wall ms of the call up to a synchronise, ms between events around it, host ms until it returns)"""
        t0 = time.perf_counter()
        self.ev[0].record()
        self.enqueue_c()
        t1 = time.perf_counter()
        self.ev[1].record()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return (t2 - t0) * 1e3, self.ev[0].elapsed_time(self.ev[1]), (t1 - t0) * 1e3

    def route_b(self):
        """-> (row-node store ms, loop ms, commitments); after an extend()."""
        t0 = time.perf_counter()
        dah = da.DataAvailabilityHeader([r.tobytes() for r in self.d.row_roots[0].cpu().numpy()],
                                        [r.tobytes() for r in self.d.col_roots[0].cpu().numpy()])
        cacher = inc.EDSSubTreeRootCacher(K, self.d.eds[0], self.ctx)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out = [inc.get_commitment(cacher, dah, int(f), int(c)) for s, f, c in self.recs if s == 0]
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, out

    def route_d(self, check):
        t0 = time.perf_counter()
        self.d.load_txs([self.txs] * self.n)
        if check:
            self.enqueue_c()
        self.d.extend()
        dah = self.d.dah.cpu()
        if check:
            flags = self.c_sq.cpu()
            assert not flags.any()
        return (time.perf_counter() - t0) * 1e3, dah


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--blocks", type=int, nargs="*", default=[1, 64])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("blob_commit_bench: no GPU")
    ctx = da.Context(0)
    txs = full_block()
    for n in args.blocks:
        b = Bench(ctx, txs, n)
        wa, wc, dc, hc, d0, d1 = [], [], [], [], [], []
        for it in range(args.warmup + args.repeats):
            torch.cuda.synchronize()
            a = b.route_a()
            torch.cuda.synchronize()
            c = b.route_c()
            torch.cuda.synchronize()
            x0, dah0 = b.route_d(False)
            torch.cuda.synchronize()
            x1, dah1 = b.route_d(True)
            assert torch.equal(dah0, dah1)
            if it >= args.warmup:
                for lst, v in ((wa, a), (wc, c[0]), (dc, c[1]), (hc, c[2]), (d0, x0), (d1, x1)):
                    lst.append(v)
        torch.cuda.synchronize()
        same = bool((b.c_out.cpu().numpy() == b.a_out).all()) and not bool(b.c_st.cpu().any())
        row = {"measure": "commitments", "k": K, "blocks": n, "blobs": b.nb, "blob_shares": b.nshares,
               "a_upload_bytes": int(b.a_shares.size + b.a_ns.size + b.a_cnt.size * 4),
               "c_upload_bytes": int(b.recs.size * 8), **stats("a_host_route_wall_ms", wa),
               **stats("c_device_wall_ms", wc), **stats("c_event_span_ms", dc), **stats("c_call_returns_ms", hc),
               "a_over_c_wall": round(statistics.median(wa) / statistics.median(wc), 3),
               **stats("d_txs_to_dah_wall_ms", d0), **stats("d_with_commitments_wall_ms", d1),
               "d_added_ms_median": round(statistics.median(d1) - statistics.median(d0), 4),
               "a_equals_c": same, "repeats": args.repeats}
        if n == 1:
            store, loop, got = [], [], None
            for _ in range(3):
                s, l, got = b.route_b()
                store.append(s)
                loop.append(l)
            row.update({**stats("b_row_node_store_ms", store), **stats("b_get_commitment_loop_ms", loop),
                        "b_equals_c": bool(b"".join(got) == b.c_out.cpu().numpy().tobytes())})
        assert same, "routes a and c disagree"
        print(json.dumps(row), flush=True)
        del b
    ctx.close()


if __name__ == "__main__":
    main()
