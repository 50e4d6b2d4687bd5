#!/usr/bin/env python3
"""DeviceSquares.load_txs with the layout made on the host (plan="host":
dagpu_square_plan on a thread pool, then dagpu_square_write_device) against the
layout made on the GPU (plan="device": dagpu_square_construct_device), on full
128 x 128 blocks (full_block() of tests/square_corpus.py: 2,000 normal + 2,000
blob txs; a batch is the same block n times):

  1 block     plan="host" | plan="device"
  256 blocks  plan="host" with 1 and with 16 threads | plan="device"
  the same followed by extend() and the DAHs' download: blocks -> DAHs per second
  the planner's kernels alone (dagpu_square_construct_device on txs already in
  HBM, between HIP events), and the planner without the writer

--host-lib PATH: dagpu_square_plan of one full block timed in turns with the
same call of another build of the library (the parent commit's), to show what
the host planner costs in this run against that build.
--phases: the loaded library (DAGPU_LIB) is a measurement build
(-DDAGPU_PLAN_CLOCKS, tools/build_variant.sh): only the kernels-alone runs,
with the phases of one block's workgroup from the wall clock that build leaves
in the workspace (median over the blocks; layout includes the one-lane
NextShareIndex walk).

The routes take turns inside every repeat.  Wall times are host clocks around a
synchronised device.  --timeline: only device-planned batches, for a kernel trace.
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
from celestia_da import _abi, da, device, square as sq  # noqa: E402
from square_corpus import full_block  # noqa: E402

K = 128


def stats(v):
    return {"median_ms": round(statistics.median(v) * 1e3, 3), "min_ms": round(min(v) * 1e3, 3),
            "max_ms": round(max(v) * 1e3, 3)}


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def host_plan_ms(libs, txs, rounds=5, calls=40):
    """Best mean time of dagpu_square_plan on one full block, the libraries taking turns."""
    import ctypes
    buf, lens = sq._pack(txs)
    plan = np.empty(1 << 20, np.uint8)
    need, k = ctypes.c_size_t(0), ctypes.c_uint32(0)
    fns = []
    for path in libs:
        f = ctypes.CDLL(path).dagpu_square_plan
        f.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32] + \
                     [ctypes.c_void_p] * 2 + [ctypes.c_size_t] + [ctypes.c_void_p] * 2
        fns.append(f)
    best = [1e9] * len(libs)
    for _ in range(rounds):
        for j, f in enumerate(fns):
            t = time.perf_counter()
            for _ in range(calls):
                rc = f(None, _abi.addr(buf), _abi.addr(lens), len(txs), K, 64, None, _abi.addr(plan), plan.size,
                       ctypes.addressof(need), ctypes.addressof(k))
                assert rc == 0
            best[j] = min(best[j], (time.perf_counter() - t) / calls)
    return [round(b * 1e3, 3) for b in best]


def kernels_alone(ctx, txs, n, repeats, write, phases=False):
    """The enqueue of the planner (and writer) on txs already in HBM, between events."""
    L = ctx._L
    src, offs, ntx, lens = sq.pack_blocks([txs] * n)
    d_src = torch.from_numpy(src).cuda()
    cap = L.dagpu_square_plan_device_arena_size(n, int(lens.size), K)
    arena = torch.empty((cap,), dtype=torch.uint8, device="cuda")
    rec = torch.empty((n * _abi.PLAN_RECORD_BYTES,), dtype=torch.uint8, device="cuda")
    status = torch.zeros((max(n, 4),), dtype=torch.int32, device="cuda")
    ws = torch.empty((L.dagpu_square_plan_device_workspace_size(n, int(lens.size), K),), dtype=torch.uint8, device="cuda")
    out = torch.empty((n * K * K * 512,), dtype=torch.uint8, device="cuda") if write else None
    s = torch.cuda.current_stream()
    ms = []
    for _ in range(repeats + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        common = (_abi.addr(d_src), _abi.addr(offs), int(src.size), _abi.addr(ntx), _abi.addr(lens), K, 64,
                  _abi.addr(arena), cap, _abi.addr(rec))
        if write:
            rc = L.dagpu_square_construct_device(ctx.handle, K, n, *common, _abi.addr(out), K * K * 512, K * 512,
                                                 _abi.addr(status), _abi.addr(ws), s.cuda_stream)
        else:
            rc = L.dagpu_square_plan_device(ctx.handle, n, *common, _abi.addr(status), _abi.addr(ws), s.cuda_stream)
        assert rc == 0, ctx.last_error()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / 1e3)
    assert (status[:n].cpu() == 0).all()
    r = stats(ms[1:])
    if not phases:
        return r
    # a measurement build: the last 64 n bytes of the workspace hold the 100 MHz
    # wall clock at the block's start and after each phase
    clk = ws[-64 * n:].cpu().numpy().view(np.uint64).reshape(n, 8).astype(np.int64)
    for i, name in enumerate(("scan", "fill", "sort", "layout", "pfb", "emit")):
        r["block_" + name + "_us"] = round(float(np.median(clk[:, i + 1] - clk[:, i])) / 100, 1)
    r["block_total_us"] = round(float(np.median(clk[:, 6] - clk[:, 0])) / 100, 1)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeline", action="store_true")
    ap.add_argument("--phases", action="store_true")
    ap.add_argument("--host-lib", default=None)
    a = ap.parse_args()
    ctx = da.Context(0)
    txs = full_block()
    k, ods = sq.construct_native(txs)
    assert k == K
    if a.phases:
        for n in (1, a.blocks):
            print(json.dumps({"what": "planner kernels + writer, measurement build, between events", "blocks": n,
                              **kernels_alone(ctx, txs, n, a.repeats, True, phases=True)}), flush=True)
        return
    libs = [_abi.LIB_PATH] + ([a.host_lib] if a.host_lib else [])
    ms = host_plan_ms(libs, txs)
    r = {"what": "dagpu_square_plan of one full block on the host", "ms": ms[0]}
    if a.host_lib:
        r["ms_other_build"] = ms[1]
        r["other_build"] = os.path.basename(a.host_lib)
    print(json.dumps(r), flush=True)
    if a.timeline:
        d = device.DeviceSquares(K, a.blocks, ctx=ctx, in_place=True)
        for _ in range(a.repeats):
            d.load_txs([txs] * a.blocks, plan="device")
        torch.cuda.synchronize()
        return
    for n, repeats in ((1, 4 * a.repeats), (a.blocks, a.repeats)):
        blocks = [txs] * n
        d = device.DeviceSquares(K, n, ctx=ctx, in_place=True)
        routes = [("host, 16 threads", dict(plan="host", threads=16)), ("device", dict(plan="device"))]
        if n > 1:
            routes.insert(0, ("host, 1 thread", dict(plan="host", threads=1)))
        want = None
        for name, kw in routes:  # warm-up, and the routes give the same squares and DAHs
            d.load_txs(blocks, **kw)
            d.extend()
            torch.cuda.synchronize()
            q0 = d.q0()[0].cpu().numpy().reshape(-1)
            assert (q0 == ods).all(), name
            dah = d.dah.cpu()
            assert want is None or torch.equal(dah, want), name
            want = dah
        load = {name: [] for name, _ in routes}
        full = {name: [] for name, _ in routes}
        for _ in range(repeats):
            for name, kw in routes:
                load[name].append(timed(lambda: d.load_txs(blocks, **kw)))
            for name, kw in routes:
                def run():
                    d.load_txs(blocks, **kw)
                    d.extend()
                    d.dah.cpu()
                full[name].append(timed(run))
        for name, _ in routes:
            r = {"what": "load_txs", "blocks": n, "plan": name, **stats(load[name])}
            r["blocks_per_s"] = round(n / statistics.median(load[name]), 1)
            print(json.dumps(r), flush=True)
        for name, _ in routes:
            r = {"what": "load_txs + extend + DAHs to the host", "blocks": n, "plan": name, **stats(full[name])}
            r["blocks_per_s"] = round(n / statistics.median(full[name]), 1)
            print(json.dumps(r), flush=True)
        del d
        for write in (False, True):
            r = {"what": "planner kernels" + (" + writer" if write else "") + ", txs resident, between events",
                 "blocks": n, **kernels_alone(ctx, txs, n, repeats, write)}
            print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
