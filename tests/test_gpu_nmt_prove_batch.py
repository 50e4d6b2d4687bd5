"""Batched nmt range proofs from a resident square, rows and columns
(dagpu_col_nodes_device, dagpu_nmt_prove_batch_device; inclusion.EDSAxisNodes,
device.nmt_prove_batch_device, proof.prove_ranges).

The specification is nmt's recursive buildRangeProof over trees hashed with the
oracle's pure-Python nmt hasher (pyref); for rows also proof.prove_row_ranges,
the host loop the batched call replaces.  Round trips feed the producer's
outputs straight to device.nmt_verify_batch_device on the same stream."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))
import pyref  # noqa: E402
from celestia_da import _abi, da, device, inclusion, proof, synth  # noqa: E402

pytestmark = pytest.mark.gpu

OK, ERR_PROOF, ERR_ARG = _abi.OK, _abi.ERR_PROOF, _abi.ERR_ARG
PARITY = b"\xff" * 29


@pytest.fixture(scope="module")
def ctx():
    c = da.Context(0)
    yield c
    c.close()


class Square:
    """One extended square on the device with both node stores, and (for the
    small widths) every tree of both axes rebuilt with pyref."""

    def __init__(self, ctx, k, seed, reference=True):
        self.k, self.w = k, 2 * k
        w = self.w
        self.ods = synth.random_blob_square(k, seed)
        self.sq = device.DeviceSquares(k, 1, ctx=ctx)
        self.sq.load_ods(np.ascontiguousarray(self.ods).reshape(1, -1))
        self.sq.extend()
        torch.cuda.synchronize()
        assert int(self.sq.status[0]) == 0
        self.nodes = inclusion.EDSAxisNodes(k, self.sq.eds[0], ctx)
        self.roots = torch.cat([self.sq.row_roots[0].reshape(-1), self.sq.col_roots[0].reshape(-1)])
        if not reference:
            return
        self.eds = self.sq.eds[0].cpu().numpy().reshape(w * w, 512)
        cell = [self.eds[i].tobytes() for i in range(w * w)]
        self.ns = [cell[r * w + c][:29] if r < k and c < k else PARITY for r in range(w) for c in range(w)]
        leaf = [pyref.leaf(self.ns[i], cell[i]) for i in range(w * w)]
        # leaves[axis][index]: the leaf nodes of one tree; the same node serves both axes
        self.leaves = [[leaf[i * w:(i + 1) * w] for i in range(w)], [leaf[i::w] for i in range(w)]]
        self._sub = {}

    def subroot(self, axis, index, lo, hi):
        """nmt computeRoot of leaves [lo, hi) of one tree (full trees split in halves)."""
        key = (axis, index, lo, hi)
        if key not in self._sub:
            if hi - lo == 1:
                self._sub[key] = self.leaves[axis][index][lo]
            else:
                mid = (lo + hi) // 2
                self._sub[key] = pyref.node(self.subroot(axis, index, lo, mid), self.subroot(axis, index, mid, hi))
        return self._sub[key]

    def range_proof(self, axis, index, start, end):
        """nmt buildRangeProof: roots of the maximal subtrees disjoint from
        [start, end), left to right."""
        out = []

        def rec(lo, hi):
            if hi <= start or lo >= end:
                out.append(self.subroot(axis, index, lo, hi))
                return
            if hi - lo == 1:
                return
            mid = (lo + hi) // 2
            rec(lo, mid)
            rec(mid, hi)

        rec(0, self.w)
        return out

    def cells(self, axis, index, start, end):
        w = self.w
        return [index * w + j if axis == 0 else j * w + index for j in range(start, end)]


_squares = {}


def _square(ctx, k, reference=True):
    if k not in _squares:
        _squares[k] = Square(ctx, k, 4100 + k, reference)
    return _squares[k]


def _rec_to_node(rec):
    return rec[0:29].tobytes() + rec[32:61].tobytes() + rec[64:96].tobytes()


# ---- column inner levels -----------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_column_inner_levels(ctx, k):
    s = _square(ctx, k)
    w = s.w
    L = ctx._L
    assert L.dagpu_col_nodes_size(k) == L.dagpu_row_nodes_size(k) - w * w * 96 == s.nodes.col_inner.numel()
    assert L.dagpu_col_nodes_workspace_size(k) > 0 and L.dagpu_col_nodes_size(3) == 0
    torch.cuda.synchronize()
    recs = s.nodes.col_inner.cpu().numpy().reshape(-1, 96)
    base, checked = 0, 0
    for lvl in range(1, w.bit_length()):
        per = w >> lvl
        for col in range(w):
            for p in range(per):
                got = _rec_to_node(recs[base + col * per + p])
                assert got == s.subroot(1, col, p << lvl, (p + 1) << lvl), (k, lvl, col, p)
                checked += 1
        base += w * per
    assert base == len(recs) and checked == w * (w - 1)
    # the top level is the column roots of the extend call
    col_roots = s.sq.col_roots[0].cpu().numpy()
    top = s.nodes.col_roots().cpu().numpy()
    assert [_rec_to_node(top[c]) for c in range(w)] == [col_roots[c].tobytes() for c in range(w)]
    # the namespace fields are zero padded to 32 B, as in the row store
    assert not recs[:, 29:32].any() and not recs[:, 61:64].any()


# ---- exhaustive production ---------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_every_range_of_every_tree(ctx, k):
    s = _square(ctx, k)
    w = s.w
    # axes alternate inside the batch; ranges in (start, end) order, so the
    # whole-tree range [0, w) sits between [0, w - 1) and [1, 2)
    reqs = [(axis, index, a, b) for index in range(w) for a in range(w) for b in range(a + 1, w + 1)
            for axis in (0, 1)]
    assert len(reqs) == 2 * w * (w * (w + 1) // 2)
    nodes, ns, shares, desc = device.nmt_prove_batch_device(s.nodes, reqs, eds=s.nodes.eds, ctx=ctx)
    torch.cuda.synchronize()
    nodes, ns, shares = nodes.cpu().numpy().tobytes(), ns.cpu().numpy().tobytes(), shares.cpu().numpy().reshape(-1, 512)
    want = [s.range_proof(*r) for r in reqs]
    node_off = leaf_off = 0
    for i, (r, wn) in enumerate(zip(reqs, want)):
        axis, index, a, b = r
        assert desc[i].tolist() == [a, b, b - a, leaf_off, len(wn), node_off, i, axis * w + index], r
        assert len(wn) == bin(a).count("1") + (w.bit_length() - 1) - bin(b - 1).count("1")
        assert nodes[90 * node_off:90 * (node_off + len(wn))] == b"".join(wn), r
        cells = s.cells(*r)
        assert ns[29 * i:29 * (i + 1)] == s.ns[cells[0]], r
        assert (shares[leaf_off:leaf_off + b - a] == s.eds[cells]).all(), r
        node_off += len(wn)
        leaf_off += b - a
    assert len(nodes) == 90 * node_off and len(shares) == leaf_off
    # the cases the closed form could get wrong
    whole = [i for i, r in enumerate(reqs) if (r[2], r[3]) == (0, w)]
    assert len(whole) == 2 * w and all(desc[i][4] == 0 for i in whole)
    if k > 1:
        assert all(desc[i - 2][4] > 0 and desc[i + 2][4] > 0 for i in whole[2:-2])
    assert any(r[3] == w and r[2] > 0 for r in reqs)                 # ranges ending at 2k
    if k > 1:
        assert any(r[2] < k < r[3] for r in reqs)                    # across the Q0 | parity boundary
    # rows also equal the host loop this call replaces
    rows = [(i, r) for i, r in enumerate(reqs) if r[0] == 0]
    cacher = inclusion.EDSSubTreeRootCacher(k, s.nodes.eds, ctx)
    for (i, r), p in zip(rows, proof.prove_row_ranges(cacher, [(r[1], r[2], r[3]) for _, r in rows])):
        assert (p.start, p.end, p.nodes) == (r[2], r[3], want[i]), r
    # the convenience form: both axes, one copy to the host
    some = reqs[::7]
    got = proof.prove_ranges(s.nodes, some)
    assert [(p.start, p.end, p.nodes) for p in got] == [(r[2], r[3], want[i]) for i, r in list(enumerate(reqs))[::7]]
    # without the square: nodes and namespaces only
    n2, ns2, sh2, d2 = device.nmt_prove_batch_device(s.nodes, reqs, ctx=ctx)
    assert sh2 is None and (d2 == desc).all()
    assert n2.cpu().numpy().tobytes() == nodes and ns2.cpu().numpy().tobytes() == ns


# ---- produce -> verify on one stream -----------------------------------------------------

def _verifiable_requests(k):
    """Every cell as a single-cell sample on both axes, and every range inside
    the parity half [k, 2k) of every tree: one namespace per range."""
    w = 2 * k
    reqs = [(axis, i, j, j + 1) for axis in (0, 1) for i in range(w) for j in range(w)]
    reqs += [(axis, i, a, b) for axis in (0, 1) for i in range(w) for a in range(k, w) for b in range(a + 1, w + 1)
             if b - a > 1]
    return reqs


def test_round_trip_on_one_stream(ctx):
    k = 16
    s = _square(ctx, k, reference=False)
    reqs = _verifiable_requests(k)
    assert len(reqs) == 2 * 1024 + 2 * 32 * (16 * 17 // 2 - 16)
    nodes, ns, shares, desc = device.nmt_prove_batch_device(s.nodes, reqs, eds=s.nodes.eds, ctx=ctx)
    st = device.nmt_verify_batch_device(desc, ns, shares, 512, nodes, s.roots, ctx=ctx)
    assert st.is_cuda and all(t.is_cuda for t in (nodes, ns, shares))
    st = st.cpu().numpy()
    assert len(st) == len(reqs) and (st == OK).all(), np.nonzero(st != OK)[0][:8]
    # single-cell row samples may read their leaf from the square itself
    rows = np.array([i for i, r in enumerate(reqs) if r[0] == 0 and r[3] - r[2] == 1])
    d2 = desc[rows].copy()
    d2[:, 3] = [reqs[i][1] * 2 * k + reqs[i][2] for i in rows]
    st = device.nmt_verify_batch_device(d2, ns, s.nodes.eds, 512, nodes, s.roots, ctx=ctx).cpu().numpy()
    assert (st == OK).all()
    # one flipped byte of one emitted node fails exactly the proofs that hold it
    victim = int(desc[len(reqs) // 3][5]) + 1
    nodes[90 * victim + 70] ^= 1
    hit = (desc[:, 5] <= victim) & (victim < desc[:, 5] + desc[:, 4])
    assert hit.sum() == 1
    st = device.nmt_verify_batch_device(desc, ns, shares, 512, nodes, s.roots, ctx=ctx).cpu().numpy()
    assert (st[hit] == ERR_PROOF).all() and (st[~hit] == OK).all()


def test_workload_width_round_trip(ctx):
    k = 128
    w = 2 * k
    s = Square(ctx, k, 128128, reference=False)
    rng = random.Random(128)
    reqs = []
    for i in range(4096):
        axis, index = rng.randrange(2), rng.randrange(w)
        if i % 2:
            a = rng.randrange(w)
            reqs.append((axis, index, a, a + 1))
        else:
            a = rng.randrange(k, w)
            reqs.append((axis, index, a, rng.randrange(a + 1, w + 1)))
    nodes, ns, shares, desc = device.nmt_prove_batch_device(s.nodes, reqs, eds=s.nodes.eds, ctx=ctx)
    st = device.nmt_verify_batch_device(desc, ns, shares, 512, nodes, s.roots, ctx=ctx).cpu().numpy()
    assert len(st) == 4096 and (st == OK).all(), np.nonzero(st != OK)[0][:8]
    assert {r[0] for r in reqs} == {0, 1} and nodes.numel() == 90 * int(desc[:, 4].sum())


# ---- validation --------------------------------------------------------------------------

def test_invalid_requests_fail_the_call_and_touch_nothing(ctx):
    k = 4
    s = _square(ctx, k)
    w = s.w
    dev = s.nodes.nodes.device
    good = [(0, 1, 2, 5), (1, 3, 0, w), (1, 0, 7, 8), (0, 7, 0, 1)]
    n_nodes = sum(len(s.range_proof(*r)) for r in good)
    n_cells = sum(r[3] - r[2] for r in good)
    fill, word = 0xA5, -0x5A5A5A5A5A5A5A5B
    L = ctx._L
    ws = torch.empty(L.dagpu_nmt_prove_workspace_size(len(good)), dtype=torch.uint8, device=dev)

    def call(reqs, nodes_cap=n_nodes, shares_cap=n_cells, col=True, want_shares=True):
        req = np.array(reqs, np.int64)
        out_nodes = torch.full((90 * n_nodes + 90,), fill, dtype=torch.uint8, device=dev)
        out_ns = torch.full((29 * len(reqs),), fill, dtype=torch.uint8, device=dev)
        out_sh = torch.full((512 * n_cells + 512,), fill, dtype=torch.uint8, device=dev)
        desc = np.full((len(reqs), 8), word, np.int64)
        total = ctypes.c_size_t(12345)
        rc = L.dagpu_nmt_prove_batch_device(
            ctx.handle, k, len(reqs), req.ctypes.data, s.nodes.eds.data_ptr(), s.nodes.nodes.data_ptr(),
            s.nodes.col_inner.data_ptr() if col else None, out_nodes.data_ptr(), nodes_cap, out_ns.data_ptr(),
            out_sh.data_ptr() if want_shares else None, shares_cap, desc.ctypes.data, ctypes.byref(total),
            ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        untouched = (bool((out_nodes == fill).all()) and bool((out_ns == fill).all()) and bool((out_sh == fill).all())
                     and bool((desc == word).all()) and total.value == 12345)
        return rc, untouched, total.value, out_nodes, out_sh

    rc, untouched, total, out_nodes, out_sh = call(good)
    assert rc == OK and not untouched and total == n_nodes
    # exact capacities: the spare node and cell behind them stay as they were
    assert bool((out_nodes[90 * n_nodes:] == fill).all()) and bool((out_sh[512 * n_cells:] == fill).all())
    assert not bool((out_nodes[:90 * n_nodes] == fill).all())
    bad = [(2, 0, 0, 1), (-1, 0, 0, 1), (0, w, 0, 1), (1, -1, 0, 1), (0, 0, -1, 1), (0, 0, 3, 3), (1, 0, 4, 3),
           (0, 0, 0, w + 1), (1, 0, w, w + 1), (0, 0, 0, 0)]
    for b in bad:
        for at in (0, len(good) - 1):
            reqs = list(good)
            reqs[at] = b
            rc, untouched, _, _, _ = call(reqs)
            assert rc == ERR_ARG and untouched, (b, at)
            assert "proof request %d" % at in ctx.last_error()
    rc, untouched, _, _, _ = call(good, col=False)                       # a column request, no column nodes
    assert rc == ERR_ARG and untouched
    rc, untouched, _, _, _ = call(good, nodes_cap=n_nodes - 1)           # one node too few
    assert rc == ERR_ARG and untouched
    rc, untouched, _, _, _ = call(good, shares_cap=n_cells - 1)          # one cell too few
    assert rc == ERR_ARG and untouched
    # rows alone need no column nodes; without shares their capacity is not looked at
    rc, untouched, total, _, out_sh = call([r for r in good if r[0] == 0], col=False, want_shares=False, shares_cap=0)
    assert rc == OK and total == sum(len(s.range_proof(*r)) for r in good if r[0] == 0)
    assert bool((out_sh == fill).all())
    with pytest.raises(da.DAError) as e:
        proof.prove_ranges(s.nodes, [(0, 0, 0, w + 1)])
    assert e.value.code == ERR_ARG
