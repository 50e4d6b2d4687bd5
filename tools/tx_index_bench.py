#!/usr/bin/env python3
"""The tx index of 64 full 128 x 128 blocks (2,000 normal + 2,000 blob txs each)
that are resident in HBM, against what there was before it.  The routes of each
group take turns inside every repeat:

  table   t_dev   dagpu_square_scan_device + dagpu_square_units_device, then D2H
                  of the unit summaries (the table itself stays in HBM)
          t_host  the route before the index: scan + dagpu_square_read_device of
                  both compact namespaces, D2H of that payload, its offsets and
                  the records, then dagpu_compact_units over every sequence on
                  one host thread
  read    r_1     DeviceSquares.read_tx_units of one tx
          r_1024  of 1,024 txs spread over the blocks
          r_all   DeviceSquares.read_txs: every tx stream downloaded and walked
  proofs  p_1024  DeviceSquares.tx_proofs of 1,024 txs spread over the blocks
                  (the proof store is built before the clock starts, as it is
                  for share_proofs)
          p_ref   proof.new_tx_inclusion_proof, which rebuilds the block's
                  square from its txs for every proof: --ref-proofs calls are
                  timed and the figure for 1,024 is extrapolated from their
                  mean (named so in the output)

Device times are HIP events around a route's device part, wall times a host
clock around work that ends in a synchronise.  Downloads of the table routes go
into pinned memory allocated before any clock starts.  Once, before the timed
part, the two table routes must count the same units and read_tx_units must
return what read_txs returns.  Kernel times come from a rocprofv3 kernel trace
in a run of its own: tools/tx_index_bench.sh.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from celestia_da import _abi, da, device, proof, square as sq  # noqa: E402
from square_read_bench import K, ODS, SHARES, stats, tx_pool  # noqa: E402


class Table:
    """The two table routes over preallocated buffers."""

    def __init__(self, ctx, d, unit_cap):
        self.ctx, self.L, self.n, self.cap = ctx, ctx._L, d.n, unit_cap
        self.buf, self.stride, self.pitch = d._resident()
        n, L = self.n, self.L
        dev = dict(dtype=torch.uint8, device="cuda")
        self.records = torch.empty((n, SHARES, 64), **dev)
        self.summary = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        self.units = torch.empty((n, unit_cap, 32), **dev)
        self.usum = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        self.scan_ws = torch.empty((L.dagpu_square_scan_workspace_size(K, n),), **dev)
        self.units_ws = torch.empty((L.dagpu_square_units_workspace_size(K, n),), **dev)
        self.read_ws = torch.empty((L.dagpu_square_read_workspace_size(K, n, SHARES, 0),), **dev)
        self.selected = torch.empty((n * SHARES,), dtype=torch.int32, device="cuda")
        self.offsets = torch.empty((n * SHARES,), dtype=torch.int64, device="cuda")
        self.totals = torch.empty((3,), dtype=torch.int64, device="cuda")
        self.h_summary = np.zeros((n, 8), np.int32)
        self.h_usum = torch.empty((n, 8), dtype=torch.int32).pin_memory()
        self.scan(True)
        self.bytes = int(self.h_summary[:, 6].astype(np.int64).sum())
        self.top = int(self.h_summary[:, 3].max())
        self.payload = torch.empty((self.bytes,), **dev)
        self.h_payload = torch.empty((self.bytes,), dtype=torch.uint8).pin_memory()
        self.h_records = torch.empty((n, self.top, 64), dtype=torch.uint8).pin_memory()
        self.h_selected = torch.empty((n * SHARES,), dtype=torch.int32).pin_memory()
        self.h_offsets = torch.empty((n * SHARES,), dtype=torch.int64).pin_memory()
        self.off = np.empty(unit_cap + 1, np.uint64)
        self.len = np.empty(unit_cap + 1, np.uint64)
        self.ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        self.found = {}

    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    def scan(self, to_host):
        self.ctx.check(self.L.dagpu_square_scan_device(
            self.ctx.handle, K, self.n, self.buf.data_ptr(), self.stride, self.pitch, SHARES, self.records.data_ptr(),
            self.summary.data_ptr(), self.h_summary.ctypes.data if to_host else None, self.scan_ws.data_ptr(),
            self.stream()))

    def t_dev(self):
        t0 = time.perf_counter()
        self.ev[0].record()
        self.scan(False)
        self.ev[1].record()
        self.ctx.check(self.L.dagpu_square_units_device(
            self.ctx.handle, K, self.n, self.buf.data_ptr(), self.stride, self.pitch, SHARES, self.records.data_ptr(),
            self.summary.data_ptr(), self.cap, self.units.data_ptr(), self.usum.data_ptr(), None,
            self.units_ws.data_ptr(), self.stream()))
        self.ev[2].record()
        self.h_usum.copy_(self.usum, non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        s = self.h_usum.numpy()
        assert (s[:, 0] == _abi.UNITS_OK).all(), s[:, :2]
        self.found["t_dev"] = int(s[:, 2].sum())
        return self.ev[0].elapsed_time(self.ev[2]), (t1 - t0) * 1e3, self.ev[1].elapsed_time(self.ev[2])

    def t_host(self):
        t0 = time.perf_counter()
        self.ev[0].record()
        self.scan(False)
        self.ctx.check(self.L.dagpu_square_read_device(
            self.ctx.handle, K, self.n, self.buf.data_ptr(), self.stride, self.pitch, SHARES,
            self.records.data_ptr(), self.summary.data_ptr(), None, 0, _abi.READ_COMPACT, self.selected.data_ptr(),
            self.offsets.data_ptr(), self.totals.data_ptr(), self.payload.data_ptr(), self.bytes,
            self.read_ws.data_ptr(), self.stream()))
        self.ev[1].record()
        nsel, nbytes, over = (int(v) for v in self.totals.cpu())  # waits: the sizes of the downloads
        assert not over and nsel > 0
        self.h_payload[:nbytes].copy_(self.payload[:nbytes], non_blocking=True)
        self.h_selected[:nsel].copy_(self.selected[:nsel], non_blocking=True)
        self.h_offsets[:nsel].copy_(self.offsets[:nsel], non_blocking=True)
        self.h_records.copy_(self.records[:, :self.top], non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        rec = self.h_records.numpy().view(sq.seq_dtype()).reshape(self.n, self.top)
        base, total, n = self.h_payload.data_ptr(), 0, ctypes.c_size_t(0)
        slots, offs = self.h_selected[:nsel].numpy(), self.h_offsets[:nsel].numpy()
        for slot, off in zip(slots, offs):
            r = rec[int(slot) // SHARES, int(slot) % SHARES]
            rc = self.L.dagpu_compact_units(base + int(off), int(r["payload"]), int(r["reserved"]),
                                            self.off.ctypes.data, self.len.ctypes.data, self.cap + 1, ctypes.byref(n))
            assert rc == 0
            total += n.value
        t2 = time.perf_counter()
        self.found["t_host"] = total
        return self.ev[0].elapsed_time(self.ev[1]), (t2 - t0) * 1e3, (t2 - t1) * 1e3


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--read-repeats", type=int, default=3, help="repeats of the read and proof groups")
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--ref-proofs", type=int, default=2)
    ap.add_argument("--table-only", action="store_true", help="the table routes only (kernel-trace runs)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tx_index_bench: no GPU")
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
    units, summary = d.tx_table()
    assert (summary[:, 0] == _abi.UNITS_OK).all() and (summary[:, 2] == 4000).all()
    t = Table(ctx, d, int(units.shape[1]))
    out = {"t_dev": [], "t_host": []}
    for it in range(args.warmup + args.repeats):
        for x in out:
            torch.cuda.synchronize()
            res = getattr(t, x)()
            if it >= args.warmup:
                out[x].append(res)
    assert t.found["t_dev"] == t.found["t_host"] == 4000 * n
    compact_shares = int(sum(int(r["count"]) for i in range(n) for r in
                             t.h_records.numpy().view(sq.seq_dtype()).reshape(n, t.top)[i, :int(t.h_summary[i, 3])]
                             if r["flags"] & 6 and not r["flags"] & 8))
    line = {"measure": "tx_index_table", "k": K, "blocks": n, "units": t.found["t_dev"], "repeats": args.repeats,
            "compact_shares": compact_shares, "compact_payload_bytes": t.bytes, "unit_cap": t.cap,
            # what the unit kernels have to move: 40 B of every share and 8 B written per share (local), those 8 B
            # read (emit), the content of the compact shares read by both walks, a 32-B record per unit
            "units_local_bytes": n * SHARES * 48 + compact_shares * 478,
            "units_emit_bytes": n * SHARES * 8 + compact_shares * 478 + t.found["t_dev"] * 32}
    line.update({**stats("t_dev_device_event_ms", [v[0] for v in out["t_dev"]]),
                 **stats("t_dev_wall_ms", [v[1] for v in out["t_dev"]]),
                 **stats("t_dev_units_only_event_ms", [v[2] for v in out["t_dev"]]),
                 **stats("t_host_device_event_ms", [v[0] for v in out["t_host"]]),
                 **stats("t_host_wall_ms", [v[1] for v in out["t_host"]]),
                 **stats("t_host_walk_ms", [v[2] for v in out["t_host"]])})
    print(json.dumps(line), flush=True)
    if args.table_only:
        ctx.close()
        return

    # selected reads against read_txs
    pairs = [((37 * j) % n, (977 * j) % 4000) for j in range(1024)]
    everything = d.read_txs()
    assert d.read_tx_units(pairs) == [(everything[i][0] + everything[i][1])[u] for i, u in pairs]
    reads = {"r_1": lambda: d.read_tx_units(pairs[:1]), "r_1024": lambda: d.read_tx_units(pairs),
             "r_all": lambda: d.read_txs()}
    got = {x: [] for x in reads}
    for it in range(1 + args.read_repeats):
        for x, fn in reads.items():
            ms, _ = wall(fn)
            if it >= 1:
                got[x].append(ms)
    line = {"measure": "tx_index_read", "blocks": n, "repeats": args.read_repeats,
            "r_1024_payload_bytes": sum(len(everything[i][0][u] if u < 2000 else everything[i][1][u - 2000])
                                        for i, u in pairs)}
    for x in reads:
        line.update(stats(x + "_wall_ms", got[x]))
    print(json.dumps(line), flush=True)
    del everything

    # tx inclusion proofs against the route that rebuilds the square
    d.extend()
    torch.cuda.synchronize()
    assert (d.status.cpu() == 0).all()
    d.tx_table()
    d.proof_store()
    torch.cuda.synchronize()
    roots = [d.dah[i].cpu().numpy().tobytes() for i in range(n)]
    p = []
    for it in range(1 + args.read_repeats):
        ms, proofs = wall(lambda: d.tx_proofs(pairs))
        if it >= 1:
            p.append(ms)
    ref = []
    for j in range(args.ref_proofs):
        i, u = pairs[j]
        ms, want = wall(lambda: proof.new_tx_inclusion_proof(blocks[i], u, ctx=ctx))
        assert proofs[j] == want, "tx_proofs differs from new_tx_inclusion_proof"
        ref.append(ms)
    assert proof.validate_batch(proofs, [roots[i] for i, _ in pairs], ctx) == [None] * len(pairs)
    line = {"measure": "tx_index_proofs", "blocks": n, "proofs": len(pairs), "repeats": args.read_repeats,
            "p_ref_calls_timed": args.ref_proofs, "p_ref_ms_per_proof_mean": round(statistics.mean(ref), 2),
            "p_ref_1024_wall_ms_extrapolated_from_that_mean": round(statistics.mean(ref) * len(pairs), 1),
            "all_1024_validate_against_the_data_roots": True}
    line.update(stats("p_1024_wall_ms", p))
    print(json.dumps(line), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
