#!/usr/bin/env python3
"""Content back out of 64 full 128 x 128 blocks (2,000 normal + 2,000 blob txs
each) that are resident in HBM, by four routes that take turns inside every
repeat:

  a  the only route before the square read: D2H of the ODS batch (8 MiB per
     square), then the Python mirror (square.deconstruct).  The mirror runs on
     --mirror-squares squares per repeat and the batch figure is extrapolated
     from its per-square time (named so in the output).
  b  D2H of the ODS batch, then the host executor dagpu_square_scan_host over
     the batch (one thread)
  c  dagpu_square_scan_device + dagpu_square_read_device of every blob and both
     tx streams, then D2H of the payload, the selection and the records
  d  the same for one blob namespace

Device times are HIP events around each route's device part, wall times a host
clock around work that ends in a synchronise.  The ODS, payload and record
downloads go into pinned memory allocated before any clock starts.  Once, after
the timed part, DeviceSquares.deconstruct of the whole batch must return every
block's txs.  Kernel times come from a rocprofv3 kernel trace in a run of its
own: tools/square_read_bench.sh.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "celestia-app_amd"))
from celestia_da import _abi, blobtx as bt, da, device, shares as sh, square as sq  # noqa: E402

K = 128
SHARES = K * K
ODS = SHARES * 512


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


def pfb_blob_sizes(tx):
    n, i, out = tx[3], 4, []
    for _ in range(n):
        v, used = sh.read_uvarint(tx[i:i + 10])
        out.append(v)
        i += used
    return out


def stats(prefix, v):
    return {prefix + "_median": round(statistics.median(v), 4), prefix + "_min": round(min(v), 4),
            prefix + "_max": round(max(v), 4)}


class Routes:
    def __init__(self, ctx, d, one_ns, mirror_squares):
        self.ctx, self.L, self.d, self.n = ctx, ctx._L, d, d.n
        self.buf, self.stride, self.pitch = d._resident()
        self.one_ns, self.mirror_squares = one_ns, mirror_squares
        n = self.n
        self.h_ods = torch.empty((n, ODS), dtype=torch.uint8).pin_memory()
        self.records = torch.empty((n, SHARES, 64), dtype=torch.uint8, device="cuda")
        self.summary = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        self.selected = torch.empty((n * SHARES,), dtype=torch.int32, device="cuda")
        self.offsets = torch.empty((n * SHARES,), dtype=torch.int64, device="cuda")
        self.totals = torch.empty((3,), dtype=torch.int64, device="cuda")
        self.scan_ws = torch.empty((self.L.dagpu_square_scan_workspace_size(K, n),), dtype=torch.uint8, device="cuda")
        self.read_ws = torch.empty((self.L.dagpu_square_read_workspace_size(K, n, SHARES, 1),), dtype=torch.uint8,
                                   device="cuda")
        self.h_summary = np.zeros((n, 8), np.int32)
        # one scan up front sizes the payload and the downloads
        self.scan(True)
        self.cap = int(self.h_summary[:, 5].astype(np.int64).sum() + self.h_summary[:, 6].astype(np.int64).sum())
        self.top = int(self.h_summary[:, 3].max())
        self.payload = torch.empty((self.cap,), dtype=torch.uint8, device="cuda")
        self.h_payload = torch.empty((self.cap,), dtype=torch.uint8).pin_memory()
        self.h_records = torch.empty((n, self.top, 64), dtype=torch.uint8).pin_memory()
        self.h_selected = torch.empty((n * SHARES,), dtype=torch.int32).pin_memory()
        self.h_offsets = torch.empty((n * SHARES,), dtype=torch.int64).pin_memory()
        self.h_records_host = np.zeros((n, SHARES), sq.seq_dtype())
        self.ns = np.frombuffer(one_ns, np.uint8).copy()
        self.ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        self.counts = {}

    def scan(self, to_host):
        self.ctx.check(self.L.dagpu_square_scan_device(
            self.ctx.handle, K, self.n, self.buf.data_ptr(), self.stride, self.pitch, SHARES, self.records.data_ptr(),
            self.summary.data_ptr(), self.h_summary.ctypes.data if to_host else None, self.scan_ws.data_ptr(),
            torch.cuda.current_stream().cuda_stream))

    def download_ods(self):
        src = self.buf.view(self.n, -1)[:, :ODS] if self.stride == ODS else \
            self.buf.view(self.n, 2 * K, 2 * K * 512)[:, :K, :K * 512]
        self.h_ods.view(self.n, K, K * 512).copy_(src.reshape(self.n, K, K * 512), non_blocking=True)

    def route_a(self):
        t0 = time.perf_counter()
        self.ev[0].record()
        self.download_ods()
        self.ev[1].record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for i in range(self.mirror_squares):
            rows = self.h_ods[i].numpy().reshape(SHARES, 512)
            txs = sq.deconstruct([sh.Share(r.tobytes()) for r in rows], pfb_blob_sizes)
            assert len(txs) == 4000
        t2 = time.perf_counter()
        per = (t2 - t1) * 1e3 / self.mirror_squares
        return self.ev[0].elapsed_time(self.ev[1]), (t1 - t0) * 1e3 + per * self.n, per

    def route_b(self):
        t0 = time.perf_counter()
        self.ev[0].record()
        self.download_ods()
        self.ev[1].record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        rc = self.L.dagpu_square_scan_host(K, self.n, self.h_ods.data_ptr(), ODS, K * 512, SHARES,
                                           self.h_records_host.ctypes.data, self.h_summary.ctypes.data)
        assert rc == 0 and (self.h_summary[:, 0] == 0).all()
        t2 = time.perf_counter()
        return self.ev[0].elapsed_time(self.ev[1]), (t2 - t0) * 1e3, (t2 - t1) * 1e3 / self.n

    def _read(self, name, ns):
        t0 = time.perf_counter()
        self.ev[0].record()
        self.scan(False)
        self.ctx.check(self.L.dagpu_square_read_device(
            self.ctx.handle, K, self.n, self.buf.data_ptr(), self.stride, self.pitch, SHARES,
            self.records.data_ptr(), self.summary.data_ptr(), ns.ctypes.data if ns is not None else None,
            1 if ns is not None else 0, _abi.READ_BLOBS | _abi.READ_COMPACT, self.selected.data_ptr(),
            self.offsets.data_ptr(), self.totals.data_ptr(), self.payload.data_ptr(), self.cap,
            self.read_ws.data_ptr(), torch.cuda.current_stream().cuda_stream))
        self.ev[1].record()
        nsel, nbytes, over = (int(v) for v in self.totals.cpu())  # waits: the sizes of the downloads
        assert not over and nsel > 0
        self.h_payload[:nbytes].copy_(self.payload[:nbytes], non_blocking=True)
        self.h_selected[:nsel].copy_(self.selected[:nsel], non_blocking=True)
        self.h_offsets[:nsel].copy_(self.offsets[:nsel], non_blocking=True)
        if ns is None:
            self.h_records.copy_(self.records[:, :self.top], non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        self.counts[name] = (nsel, nbytes)
        return self.ev[0].elapsed_time(self.ev[1]), (t1 - t0) * 1e3, 0.0

    def route_c(self):
        return self._read("c", None)

    def route_d(self):
        return self._read("d", self.ns)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--mirror-squares", type=int, default=1)
    ap.add_argument("--skip-host", action="store_true", help="routes c and d only (kernel-trace runs)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("square_read_bench: no GPU")
    ctx = da.Context(0)
    normal, blob = tx_pool()
    n = args.blocks
    blocks = []
    for i in range(n):
        a, b = i % len(normal), (7 * i) % len(blob)
        blocks.append(normal[a:] + normal[:a] + blob[b:] + blob[:b])
    d = device.DeviceSquares(K, n, ctx=ctx)
    d.load_txs(blocks)
    torch.cuda.synchronize()
    one_ns = bt.unmarshal_blob_tx(blob[0])[0].blobs[0].namespace()
    r = Routes(ctx, d, one_ns, args.mirror_squares)
    names = ["c", "d"] if args.skip_host else ["a", "b", "c", "d"]
    out = {x: [] for x in names}
    for it in range(args.warmup + args.repeats):
        for x in names:
            torch.cuda.synchronize()
            res = getattr(r, "route_" + x)()
            if it >= args.warmup:
                out[x].append(res)
    line = {"measure": "square_read", "k": K, "blocks": n, "ods_batch_bytes": n * ODS, "repeats": args.repeats,
            "sequences_per_square": int(r.h_summary[0, 3]), "blob_sequences_per_square": int(r.h_summary[0, 4]),
            "c_selected": r.counts["c"][0], "c_payload_bytes": r.counts["c"][1],
            "d_selected": r.counts["d"][0], "d_payload_bytes": r.counts["d"][1],
            # what each kernel has to move: 40 B of every share (twice: local and emit), a 64-B record per
            # sequence written by the scan and read by the select (twice), the payload read and written
            "scan_local_bytes": n * SHARES * 40, "scan_emit_bytes": n * SHARES * 40 + int(r.h_summary[:, 3].sum()) * 64,
            "select_bytes_per_pass": int(r.h_summary[:, 3].sum()) * 64, "gather_c_bytes": 2 * r.counts["c"][1]}
    for x in names:
        line.update({**stats(x + "_device_event_ms", [v[0] for v in out[x]]),
                     **stats(x + "_wall_ms", [v[1] for v in out[x]])})
    if not args.skip_host:
        line["a_wall_is_extrapolated_from_mirror_squares"] = args.mirror_squares
        line.update(stats("a_mirror_ms_per_square", [v[2] for v in out["a"]]))
        line.update(stats("b_scan_host_ms_per_square", [v[2] for v in out["b"]]))
    print(json.dumps(line), flush=True)
    if not args.skip_host:
        t0 = time.perf_counter()
        got = d.deconstruct(pfb_blob_sizes)
        t1 = time.perf_counter()
        assert got == [list(b) for b in blocks], "deconstruct does not return the blocks' txs"
        print(json.dumps({"measure": "deconstruct_batch", "blocks": n, "txs_per_block": 4000,
                          "wall_ms": round((t1 - t0) * 1e3, 2), "wall_ms_per_square": round((t1 - t0) * 1e3 / n, 3),
                          "equals_input_txs": True}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
