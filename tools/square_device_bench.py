#!/usr/bin/env python3
"""txs -> DAH for full 128 x 128 blocks (2,000 normal + 2,000 blob txs), the
shape of app.ExtendBlock, by two routes that take turns inside every repeat:

  A  dagpu_square_construct into pinned memory -> H2D of the ODS -> extend
  B  dagpu_square_plan -> H2D of the raw txs (+ the plan, inside the call)
     -> dagpu_square_write_device into Q0 of the EDS -> extend in place

  single  one block: wall time from the packed txs to the DAH on the host,
          with the host step (construct / plan) and, from HIP events, the
          device time of B's write call and of each route's extend
  batch   256 distinct blocks -> 256 DAHs: A on one host thread, B planning on
          1 and on 16 threads; blocks/s

The txs are packed (one buffer, one length array per block) in pinned memory
before any clock starts, for both routes.  Both routes must give the same
DAHs.  Kernel times come from a rocprofv3 kernel trace in a run of its own:
tools/square_device_bench.sh.
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "celestia-app_amd"))
from celestia_da import blobtx as bt, da, device, shares as sh  # noqa: E402

K = 128
ODS = K * K * 512
EDS = 4 * ODS
HBM_PEAK = 8.0e12  # bytes/s, MI355X


def tx_pool(seed=7):
    """2,000 random 300-B txs and 2,000 blob txs of one 1..3000-B blob each."""
    rng = random.Random(seed)
    normal = [rng.randbytes(300) for _ in range(2000)]
    blob = []
    for _ in range(2000):
        data = rng.randbytes(rng.randrange(1, 3001))
        pfb = (b"PFB\x01" + sh.put_uvarint(len(data))).ljust(330, b"\x00")
        blob.append(bt.marshal_blob_tx(pfb, sh.Blob.new(sh.new_namespace_v0(rng.randbytes(10)), data)))
    return normal, blob


def stats(prefix, v):
    return {prefix + "_median": round(statistics.median(v), 4), prefix + "_min": round(min(v), 4),
            prefix + "_max": round(max(v), 4)}


class Blocks:
    """n distinct blocks (rotations of one tx pool) packed in pinned memory."""

    def __init__(self, n, normal, blob):
        self.n = n
        parts = []
        for i in range(n):
            a, b = i % len(normal), (7 * i) % len(blob)
            parts.append(normal[a:] + normal[:a] + blob[b:] + blob[:b])
        self.ntx = len(parts[0])
        self.lens = np.array([[len(t) for t in p] for p in parts], np.uint64)
        self.offs = np.zeros(n + 1, np.uint64)
        self.offs[1:] = np.cumsum(self.lens.sum(axis=1))
        self.total = int(self.offs[n])
        self.src = torch.empty((self.total,), dtype=torch.uint8).pin_memory()
        v = self.src.numpy()
        for i, p in enumerate(parts):
            v[int(self.offs[i]):int(self.offs[i + 1])] = np.frombuffer(b"".join(p), np.uint8)
        self.plan_cap = 1 << 20
        self.plans = torch.empty((n, self.plan_cap), dtype=torch.uint8).pin_memory()
        self.plan_bytes = np.zeros(n, np.uint64)
        self.ods = torch.empty((n, ODS), dtype=torch.uint8).pin_memory()


class Routes:
    def __init__(self, ctx, blocks):
        self.ctx, self.L, self.b = ctx, ctx._L, blocks
        n = blocks.n
        self.a = device.DeviceSquares(K, n, ctx=ctx)
        self.q = device.DeviceSquares(K, n, ctx=ctx, in_place=True)
        self.d_src = torch.empty((blocks.total,), dtype=torch.uint8, device="cuda")
        self.ws = torch.empty((self.L.dagpu_square_write_workspace_size(n, n * blocks.plan_cap),), dtype=torch.uint8,
                              device="cuda")
        self.ptrs = np.array([blocks.plans[i].data_ptr() for i in range(n)], np.uint64)
        self.ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

    def construct(self, i):
        b = self.b
        k = ctypes.c_uint32(0)
        self.ctx.check(self.L.dagpu_square_construct(None, b.src.data_ptr() + int(b.offs[i]), b.lens[i].ctypes.data,
                                                     b.ntx, K, 64, b.ods[i].data_ptr(), ODS, ctypes.addressof(k)))
        assert k.value == K

    def plan(self, i):
        b = self.b
        k, need = ctypes.c_uint32(0), ctypes.c_size_t(0)
        rc = self.L.dagpu_square_plan(None, b.src.data_ptr() + int(b.offs[i]), b.lens[i].ctypes.data, b.ntx, K, 64,
                                      None, b.plans[i].data_ptr(), b.plan_cap, ctypes.addressof(need),
                                      ctypes.addressof(k))
        assert rc == 0 and k.value == K, (rc, k.value, need.value)
        b.plan_bytes[i] = need.value

    def route_a(self, pool=None):
        """-> (host construct ms, total wall ms, extend event ms, ODS H2D event ms)"""
        t0 = time.perf_counter()
        for i in range(self.b.n):
            self.construct(i)
        t1 = time.perf_counter()
        self.ev[0].record()
        self.a.ods.copy_(self.b.ods, non_blocking=True)
        self.ev[2].record()
        self.a.extend()
        self.ev[1].record()
        dah = self.a.dah.cpu()
        t2 = time.perf_counter()
        return ((t1 - t0) * 1e3, (t2 - t0) * 1e3, self.ev[2].elapsed_time(self.ev[1]),
                self.ev[0].elapsed_time(self.ev[2]), dah)

    def route_b(self, pool=None):
        """-> (host plan ms, total wall ms, extend event ms, write call event ms)"""
        b, n = self.b, self.b.n
        t0 = time.perf_counter()
        if pool is None:
            for i in range(n):
                self.plan(i)
        else:
            list(pool.map(self.plan, range(n)))
        t1 = time.perf_counter()
        self.d_src.copy_(b.src, non_blocking=True)
        self.ev[2].record()
        self.ctx.check(self.L.dagpu_square_write_device(
            self.ctx.handle, K, n, self.ptrs.ctypes.data, b.plan_bytes.ctypes.data, self.d_src.data_ptr(),
            b.offs.ctypes.data, b.total, self.q.eds.data_ptr(), EDS, 2 * K * 512, self.ws.data_ptr(),
            torch.cuda.current_stream().cuda_stream))
        self.ev[3].record()
        self.q.extend()
        self.ev[1].record()
        dah = self.q.dah.cpu()
        t2 = time.perf_counter()
        return ((t1 - t0) * 1e3, (t2 - t0) * 1e3, self.ev[3].elapsed_time(self.ev[1]),
                self.ev[2].elapsed_time(self.ev[3]), dah)


def alternate(fns, warmup, repeats):
    """The routes take turns inside every repeat; -> per route, lists of
    (host step ms, wall ms, extend ms, write ms) and the last DAHs."""
    out = [[] for _ in fns]
    dah = [None] * len(fns)
    for it in range(warmup + repeats):
        for j, fn in enumerate(fns):
            torch.cuda.synchronize()
            r = fn()
            if it >= warmup:
                out[j].append(r[:4])
            dah[j] = r[4]
    return out, dah


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--skip-batch", action="store_true", help="single block only (kernel-trace runs)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("square_device_bench: no GPU")
    ctx = da.Context(0)
    normal, blob = tx_pool()

    one = Blocks(1, normal, blob)
    r = Routes(ctx, one)
    (ta, tb), (dah_a, dah_b) = alternate([r.route_a, r.route_b], args.warmup, args.repeats)
    assert torch.equal(dah_a, dah_b), "routes A and B disagree"
    wall_a, wall_b = [x[1] for x in ta], [x[1] for x in tb]
    write_ms = statistics.median(x[3] for x in tb)
    plan_bytes = int(one.plan_bytes[0])
    moved = one.total + plan_bytes + ODS  # the kernel reads the txs and the plan once, writes the ODS
    spread = max(max(wall_a) - min(wall_a), max(wall_b) - min(wall_b))
    gain = statistics.median(wall_a) - statistics.median(wall_b)
    print(json.dumps({
        "measure": "single", "k": K, "txs": one.ntx, "tx_bytes": one.total, "plan_bytes": plan_bytes,
        **stats("A_wall_ms", wall_a), **stats("A_construct_ms", [x[0] for x in ta]),
        **stats("A_ods_h2d_event_ms", [x[3] for x in ta]), **stats("A_extend_event_ms", [x[2] for x in ta]),
        **stats("B_wall_ms", wall_b), **stats("B_plan_ms", [x[0] for x in tb]),
        **stats("B_write_call_event_ms", [x[3] for x in tb]), **stats("B_extend_event_ms", [x[2] for x in tb]),
        "write_call_bytes": moved,
        "write_call_fraction_of_hbm_peak": round(moved / (write_ms * 1e-3) / HBM_PEAK, 4),
        "A_minus_B_median_ms": round(gain, 4), "largest_min_max_spread_ms": round(spread, 4),
        "B_below_A_by_more_than_spread": bool(gain > spread), "repeats": args.repeats}), flush=True)
    del r, one
    if args.skip_batch:
        ctx.close()
        return

    n = args.blocks
    many = Blocks(n, normal, blob)
    r = Routes(ctx, many)
    with ThreadPoolExecutor(16) as pool:
        (ta, tb1, tb16), dahs = alternate([r.route_a, r.route_b, lambda: r.route_b(pool)], args.warmup, args.repeats)
    assert torch.equal(dahs[0], dahs[1]) and torch.equal(dahs[0], dahs[2]), "routes A and B disagree"
    assert len({bytes(d) for d in dahs[0].numpy()}) == n, "blocks are not distinct"
    out = {"measure": "batch", "k": K, "blocks": n, "tx_bytes": many.total, "plan_bytes": int(many.plan_bytes.sum())}
    for name, t in (("A_1_thread", ta), ("B_1_thread", tb1), ("B_16_threads", tb16)):
        wall = [x[1] for x in t]
        out.update({**stats(name + "_wall_ms", wall), **stats(name + "_host_step_ms", [x[0] for x in t]),
                    **stats(name + "_extend_event_ms", [x[2] for x in t]),
                    name + "_blocks_per_s": round(n / (statistics.median(wall) * 1e-3), 1)})
    write = [x[3] for x in tb16]
    out.update({**stats("B_write_call_event_ms", write),
                "B_write_call_ms_per_square": round(statistics.median(write) / n, 5),
                "B_extend_ms_per_square": round(statistics.median(x[2] for x in tb16) / n, 5),
                "write_call_fraction_of_hbm_peak": round(
                    (many.total + int(many.plan_bytes.sum()) + n * ODS) / (statistics.median(write) * 1e-3) / HBM_PEAK,
                    4), "repeats": args.repeats})
    print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
