"""Batched proof verification on the GPU (dagpu_nmt_verify_batch,
dagpu_nmt_verify_batch_device, dagpu_merkle_verify_batch; proof.validate_batch).

The specification is the library's own host verifiers: every status of a batch
must equal what dagpu_nmt_verify_inclusion / dagpu_merkle_verify returns for
that proof on the same bytes.  Trees come from the oracle's pure-Python
restatement (pyref) with nmt's split rule (the largest power of two strictly
below the length)."""
import ctypes
import hashlib
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))
import pyref  # noqa: E402
from celestia_da import _abi, da, proof, synth  # noqa: E402

pytestmark = pytest.mark.gpu

OK, ERR_PROOF, ERR_ARG = _abi.OK, _abi.ERR_PROOF, _abi.ERR_ARG
SENTINEL = 0x5A5A5A5


@pytest.fixture(scope="module")
def ctx():
    c = da.Context(0)
    yield c
    c.close()


# ---- trees and proofs with nmt's split rule ------------------------------------------

def _split(n):
    k = 1
    while k * 2 < n:
        k *= 2
    return k


def _subroot(nodes, lo, hi):
    if hi - lo == 1:
        return nodes[lo]
    k = _split(hi - lo)
    return pyref.node(_subroot(nodes, lo, lo + k), _subroot(nodes, lo + k, hi))


def _range_proof(nodes, start, end):
    """nmt buildRangeProof: roots of the maximal subtrees disjoint from
    [start, end), left to right."""
    out = []

    def rec(lo, hi):
        if hi <= start or lo >= end:
            out.append(_subroot(nodes, lo, hi))
            return
        if hi - lo == 1:
            return
        k = _split(hi - lo)
        rec(lo, lo + k)
        rec(lo + k, hi)

    rec(0, len(nodes))
    return out


class Batch:
    """Flat arrays of dagpu_nmt_verify_batch, built proof by proof."""

    def __init__(self, leaf_len):
        self.leaf_len = leaf_len
        self.desc, self.leaves, self.nodes, self.ns, self.roots = [], [], [], [], []
        self.n_leaves = self.n_nodes = 0
        self._ns, self._roots = {}, {}

    def add_leaves(self, leaves):
        off = self.n_leaves
        self.leaves.extend(leaves)
        self.n_leaves += len(leaves)
        return off

    def add(self, start, end, n_leaves, leaf_off, nodes, ns, root):
        if ns not in self._ns:
            self._ns[ns] = len(self.ns)
            self.ns.append(ns)
        if root not in self._roots:
            self._roots[root] = len(self.roots)
            self.roots.append(root)
        self.desc.append((start, end, n_leaves, leaf_off, len(nodes), self.n_nodes, self._ns[ns], self._roots[root]))
        self.nodes.extend(nodes)
        self.n_nodes += len(nodes)

    def arrays(self):
        def buf(parts):
            b = b"".join(parts)
            return np.frombuffer(b, np.uint8).copy() if b else np.zeros(16, np.uint8)
        return (np.array(self.desc, np.int64).reshape(-1, 8), buf(self.ns), len(self.ns), buf(self.leaves),
                self.n_leaves, buf(self.nodes), self.n_nodes, buf(self.roots), len(self.roots))


def _host_status(desc, ns, leaves, leaf_len, nodes, roots):
    """dagpu_nmt_verify_inclusion on every proof of the batch."""
    f = _abi.lib().dagpu_nmt_verify_inclusion
    a_ns, a_lv, a_nd, a_rt = (x.ctypes.data for x in (ns, leaves, nodes, roots))
    out = np.empty(len(desc), np.int32)
    for i, (s, e, nl, lo, nn, no, ni, ri) in enumerate(desc.tolist()):
        out[i] = f(a_ns + 29 * ni, a_lv + lo * leaf_len, nl, leaf_len, s, e, a_nd + 90 * no, nn, a_rt + 90 * ri)
    return out


def _batch_host(ctx, desc, ns, n_ns, leaves, n_leaves, leaf_len, nodes, n_nodes, roots, n_roots, status=None):
    st = np.full(len(desc), SENTINEL, np.int32) if status is None else status
    d = np.ascontiguousarray(desc)
    rc = ctx._L.dagpu_nmt_verify_batch(ctx.handle, len(d), d.ctypes.data, ns.ctypes.data, n_ns, leaves.ctypes.data,
                                       n_leaves, leaf_len, nodes.ctypes.data, n_nodes, roots.ctypes.data, n_roots,
                                       st.ctypes.data)
    return rc, st


def _batch_device(ctx, desc, ns, n_ns, leaves, n_leaves, leaf_len, nodes, n_nodes, roots, n_roots):
    dev = torch.device("cuda", 0)
    t_ns, t_lv, t_nd, t_rt = (torch.from_numpy(x).to(dev) for x in (ns, leaves, nodes, roots))
    d = np.ascontiguousarray(desc)
    st = torch.full((len(d),), SENTINEL, dtype=torch.int32, device=dev)
    proven = int(d[:, 2].clip(min=0, max=max(n_leaves, 1)).sum())
    ws = torch.empty(ctx._L.dagpu_nmt_verify_workspace_size(len(d), proven), dtype=torch.uint8, device=dev)
    rc = ctx._L.dagpu_nmt_verify_batch_device(
        ctx.handle, len(d), d.ctypes.data, t_ns.data_ptr(), n_ns, t_lv.data_ptr(), n_leaves, leaf_len,
        t_nd.data_ptr(), n_nodes, t_rt.data_ptr(), n_roots, st.data_ptr(), ws.data_ptr(),
        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, st.cpu().numpy()


def _single_ns_tree(rng, width, leaf_len=512):
    ns = b"\x00" * 19 + rng.randbytes(10)
    shares = [rng.randbytes(leaf_len) for _ in range(width)]
    return [ns] * width, shares


def _sorted_ns_tree(rng, width):
    # sorted namespaces, a run of 4 equal ones (tests/test_proof_verify_host.py)
    nss = sorted(b"\x00" * 19 + rng.randbytes(10) for _ in range(width))
    lo = width // 3
    for i in range(lo, min(width, lo + 4)):
        nss[i] = nss[lo]
    return nss, [rng.randbytes(512) for _ in range(width)]


def _add_tree(b, rng, nss, shares, tamper=True):
    """Every [start, end) of one tree, untampered and with each tampering.
    Returns the kind of every proof added: 'valid' marks an untampered range of
    one namespace."""
    width = len(shares)
    lnodes = [pyref.leaf(n, s) for n, s in zip(nss, shares)]
    root = _subroot(lnodes, 0, width)
    base = b.add_leaves(shares)
    kinds = []
    for start in range(width):
        for end in range(start + 1, width + 1):
            ns = nss[start]
            one_ns = len(set(nss[start:end])) == 1
            nodes = _range_proof(lnodes, start, end)
            n = end - start
            b.add(start, end, n, base + start, nodes, ns, root)
            kinds.append("valid" if one_ns else "multi-ns")
            if not tamper:
                continue
            bad = bytearray(shares[start])
            bad[100 % len(bad)] ^= 1
            off = b.add_leaves([bytes(bad)] + shares[start + 1:end])
            b.add(start, end, n, off, nodes, ns, root)                      # a flipped share bit
            b.add(start, end + 1, n, base + start, nodes, ns, root)          # end + 1
            if nodes:
                b.add(start, end, n, base + start,
                      nodes[1:] + nodes[:1] if len(nodes) > 1 else [bytes(90)], ns, root)  # rotated nodes
                b.add(start, end, n, base + start, nodes[:-1], ns, root)   # a dropped last node
            b.add(start, end, n, base + start, nodes, ns, bytes(90))        # a zero root
            b.add(start, end, n, base + start, nodes + [rng.randbytes(90)], ns, root)  # an extra trailing node
            b.add(-1, end, n, base + start, nodes, ns, root)                # start = -1
            b.add(start, start, 0, base + start, nodes, ns, root)           # an empty range
            kinds.extend(["tampered"] * (8 if nodes else 6))
    return kinds


def test_equivalence_corpus_host_and_device_forms(ctx):
    rng = random.Random(20260)
    b = Batch(512)
    kinds = []
    for width in (1, 2, 3, 4, 5, 6, 7, 8, 11, 13, 16, 64):
        kinds += _add_tree(b, rng, *_single_ns_tree(rng, width))
        kinds += _add_tree(b, rng, *_sorted_ns_tree(rng, width))
    # a row of an EDS at k = 8: Q0 half namespaced, parity half 0xFF (ignoreMax rule)
    k = 8
    q0 = sorted(b"\x00" * 19 + rng.randbytes(10) + rng.randbytes(483) for _ in range(k))
    par = [rng.randbytes(512) for _ in range(k)]
    lnodes = [pyref.leaf(s[:29], s) for s in q0] + [pyref.leaf(b"\xff" * 29, s) for s in par]
    root = _subroot(lnodes, 0, 2 * k)
    base = b.add_leaves(q0 + par)
    b.add(k, 2 * k, k, base + k, _range_proof(lnodes, k, 2 * k), b"\xff" * 29, root)
    b.add(2, 3, 1, base + 2, _range_proof(lnodes, 2, 3), q0[2][:29], root)
    kinds += ["valid", "valid"]
    b.add(3, 3, 0, base + 2, _range_proof(lnodes, 2, 3), q0[2][:29], root)
    b.add(-1, 1, 2, base + 2, _range_proof(lnodes, 2, 3), q0[2][:29], root)
    kinds += ["tampered", "tampered"]
    # two adjacent leaves out of namespace order: the node-hash rule rejects the pair
    nss = sorted(b"\x00" * 19 + rng.randbytes(10) for _ in range(8))
    nss[2], nss[3] = nss[3], nss[2]
    shares = [rng.randbytes(512) for _ in range(8)]
    lnodes = [pyref.leaf(n, s) for n, s in zip(nss, shares)]
    root = _subroot(lnodes, 0, 8)
    base = b.add_leaves(shares)
    b.add(2, 3, 1, base + 2, _range_proof(lnodes, 2, 3), nss[2], root)
    b.add(3, 4, 1, base + 3, _range_proof(lnodes, 3, 4), nss[3], root)
    kinds += ["tampered", "tampered"]

    desc, ns, n_ns, leaves, n_leaves, nodes, n_nodes, roots, n_roots = b.arrays()
    assert len(kinds) == len(desc)
    want = _host_status(desc, ns, leaves, 512, nodes, roots)
    rc, got = _batch_host(ctx, desc, ns, n_ns, leaves, n_leaves, 512, nodes, n_nodes, roots, n_roots)
    assert rc == OK, ctx.last_error()
    rc, got_dev = _batch_device(ctx, desc, ns, n_ns, leaves, n_leaves, 512, nodes, n_nodes, roots, n_roots)
    assert rc == OK, ctx.last_error()
    kinds = np.array(kinds)
    print(f"{len(desc)} proofs, {n_leaves} leaves, {n_nodes} nodes: host OK {int((want == OK).sum())}, "
          f"batch OK {int((got == OK).sum())}, device OK {int((got_dev == OK).sum())}, "
          f"mismatches {int((got != want).sum())} / {int((got_dev != want).sum())}")
    assert set(np.unique(want)) <= {OK, ERR_PROOF}
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(int(i), desc[i].tolist(), int(got[i]), int(want[i])) for i in bad[:5]]
    assert (got_dev == got).all(), np.nonzero(got_dev != got)[0][:5]
    assert (got[kinds == "valid"] == OK).all()
    assert (kinds == "valid").sum() > 2000
    assert (got[kinds == "tampered"] == ERR_PROOF).all()
    # a range over several namespaces does not verify: one namespace is prepended
    assert (got[kinds == "multi-ns"] == ERR_PROOF).all() and (kinds == "multi-ns").any()


@pytest.mark.parametrize("leaf_len", [0, 1, 25, 26, 33, 34, 89, 90, 512, 513])
def test_leaf_lengths_around_padding_and_block_boundaries(ctx, leaf_len):
    rng = random.Random(leaf_len)
    b = Batch(leaf_len)
    _add_tree(b, rng, *_single_ns_tree(rng, 8, leaf_len), tamper=False)
    desc, ns, n_ns, leaves, n_leaves, nodes, n_nodes, roots, n_roots = b.arrays()
    want = _host_status(desc, ns, leaves, leaf_len, nodes, roots)
    rc, got = _batch_host(ctx, desc, ns, n_ns, leaves, n_leaves, leaf_len, nodes, n_nodes, roots, n_roots)
    assert rc == OK, ctx.last_error()
    rc, got_dev = _batch_device(ctx, desc, ns, n_ns, leaves, n_leaves, leaf_len, nodes, n_nodes, roots, n_roots)
    assert rc == OK, ctx.last_error()
    assert (got == want).all() and (got_dev == want).all()
    assert (want == OK).all() and len(want) == 36


def test_descriptor_validation_before_any_launch(ctx):
    rng = random.Random(3)
    b = Batch(512)
    _add_tree(b, rng, *_single_ns_tree(rng, 4), tamper=False)
    desc, ns, n_ns, leaves, n_leaves, nodes, n_nodes, roots, n_roots = b.arrays()
    rc, st = _batch_host(ctx, desc, ns, n_ns, leaves, n_leaves, 512, nodes, n_nodes, roots, n_roots)
    assert rc == OK and (st == OK).all()
    # column: 2 n_leaves, 3 leaf_off, 4 n_nodes, 5 node_off, 6 ns_index, 7 root_index
    cases = [(3, n_leaves), (3, n_leaves - desc[5][2] + 1), (5, n_nodes + 1), (4, n_nodes + 1), (7, n_roots),
             (6, n_ns), (3, -1), (5, -1), (2, -1), (4, -1), (6, -1), (7, -1), (3, 1 << 62), (2, 1 << 62)]
    for col, val in cases:
        d = desc.copy()
        d[5][col] = val
        rc, st = _batch_host(ctx, d, ns, n_ns, leaves, n_leaves, 512, nodes, n_nodes, roots, n_roots)
        assert rc == ERR_ARG and (st == SENTINEL).all(), (col, val)
        rc, st = _batch_device(ctx, d, ns, n_ns, leaves, n_leaves, 512, nodes, n_nodes, roots, n_roots)
        assert rc == ERR_ARG and (st == SENTINEL).all(), (col, val)
    # a range the host verifier rejects fails its own proof, not the call
    d = desc.copy()
    d[5][0], d[5][1] = 1 << 62, (1 << 62) + int(d[5][2])
    rc, st = _batch_host(ctx, d, ns, n_ns, leaves, n_leaves, 512, nodes, n_nodes, roots, n_roots)
    assert rc == OK and st[5] == ERR_PROOF and (np.delete(st, 5) == OK).all()


# ---- crypto/merkle ---------------------------------------------------------------------

def _aunts(items, i):
    def rec(lo, hi):
        if hi - lo == 1:
            return []
        split = _split(hi - lo)
        if i < lo + split:
            return rec(lo, lo + split) + [pyref.rfc6962(items[lo + split:hi])]
        return rec(lo + split, hi) + [pyref.rfc6962(items[lo:lo + split])]
    return rec(0, len(items))


def _merkle_batch(ctx, desc, leaves, n_leaves, leaf_len, leaf_hashes, aunts, n_aunts, roots, n_roots):
    st = np.full(len(desc), SENTINEL, np.int32)
    rc = ctx._L.dagpu_merkle_verify_batch(
        ctx.handle, len(desc), desc.ctypes.data, leaves.ctypes.data, n_leaves, leaf_len,
        leaf_hashes.ctypes.data if leaf_hashes is not None else None, aunts.ctypes.data, n_aunts,
        roots.ctypes.data, n_roots, st.ctypes.data)
    return rc, st


def test_merkle_batch_matches_host_verifier(ctx):
    desc, leaves, hashes, aunts, roots, kinds = [], [], [], [], [], []

    def add(index, total, au, leaf, root_ix):
        desc.append((index, total, len(au), len(aunts), len(leaves), root_ix))
        aunts.extend(au)
        leaves.append(leaf)
        hashes.append(hashlib.sha256(b"\x00" + leaf).digest())

    for n in (1, 2, 3, 5, 8, 13, 32):
        rng = random.Random(n)
        items = [rng.randbytes(90) for _ in range(n)]
        roots.append(pyref.rfc6962(items))
        for i in range(n):
            au = _aunts(items, i)
            add(i, n, au, items[i], len(roots) - 1)
            kinds.append("valid")
            other = bytearray(items[i])
            other[7] ^= 0x10
            add(i, n, au, bytes(other), len(roots) - 1)                     # another leaf
            # a flipped aunt bit, or an aunt too many at n == 1
            add(i, n, [bytes([au[0][0] ^ 1]) + au[0][1:]] + au[1:] if au else [bytes(32)], items[i], len(roots) - 1)
            add(-1, n, au, items[i], len(roots) - 1)                        # index -1
            add(i, n, au + [bytes(32)] * (101 - len(au)), items[i], len(roots) - 1)  # 101 aunts
            kinds.extend(["tampered"] * 4)
    roots.append(bytes(32))
    add(0, 0, [], b"x" * 90, len(roots) - 1)   # total 0
    add(0, -1, [], b"x" * 90, len(roots) - 1)  # negative total
    add(5, 5, [], b"x" * 90, len(roots) - 1)   # index == total
    kinds.extend(["tampered"] * 3)
    d = np.array(desc, np.int64)
    lv = np.frombuffer(b"".join(leaves), np.uint8).copy()
    au = np.frombuffer(b"".join(aunts), np.uint8).copy()
    rt = np.frombuffer(b"".join(roots), np.uint8).copy()
    f = _abi.lib().dagpu_merkle_verify
    want = np.array([f(rt.ctypes.data + 32 * ri, lv.ctypes.data + 90 * li, 90, ix, tot, au.ctypes.data + 32 * ao, na)
                     for ix, tot, na, ao, li, ri in d.tolist()], np.int32)
    kinds = np.array(kinds)
    rc, got = _merkle_batch(ctx, d, lv, len(leaves), 90, None, au, len(aunts), rt, len(roots))
    assert rc == OK, ctx.last_error()
    assert (got == want).all(), np.nonzero(got != want)[0][:5]
    assert (got[kinds == "valid"] == OK).all() and (got[kinds == "tampered"] == ERR_PROOF).all()
    # with the proofs' own LeafHash fields: the right ones change nothing ...
    lh = np.frombuffer(b"".join(hashes), np.uint8).copy()
    rc, got = _merkle_batch(ctx, d, lv, len(leaves), 90, lh, au, len(aunts), rt, len(roots))
    assert rc == OK and (got == want).all()
    # ... a wrong one fails its proof alone
    valid = np.nonzero(kinds == "valid")[0]
    lh2 = lh.copy()
    for i in valid[::3]:
        lh2[32 * i + 31] ^= 0x80
    rc, got = _merkle_batch(ctx, d, lv, len(leaves), 90, lh2, au, len(aunts), rt, len(roots))
    want2 = want.copy()
    want2[valid[::3]] = ERR_PROOF
    assert rc == OK and (got == want2).all()
    # descriptors outside the buffers fail the call before any launch
    row = int(np.nonzero(d[:, 2] > 0)[0][0])  # a proof that has aunts
    for col, val in ((3, len(aunts)), (3, -1), (2, -1), (2, len(aunts) + 1), (4, len(leaves)), (4, -1),
                     (5, len(roots)), (5, -1)):
        bad = d.copy()
        bad[row][col] = val
        rc, st = _merkle_batch(ctx, bad, lv, len(leaves), 90, None, au, len(aunts), rt, len(roots))
        assert rc == ERR_ARG and (st == SENTINEL).all(), (col, val)
    # the Python list form
    items = [rng.randbytes(90) for _ in range(5)]
    root = pyref.rfc6962(items)
    ps = [proof.MerkleProof(5, i, hashlib.sha256(b"\x00" + items[i]).digest(), _aunts(items, i)) for i in range(5)]
    ps[3] = proof.MerkleProof(5, 3, bytes(32), ps[3].aunts)
    assert proof.merkle_verify_batch([(p, root, items[i]) for i, p in enumerate(ps)], ctx) == \
        [True, True, True, False, True]


# ---- samples of a resident square -------------------------------------------------------

def test_samples_from_a_resident_square(ctx):
    from celestia_da import device, inclusion
    k = 16
    w = 2 * k
    ods = synth.random_blob_square(k, 77)
    sq = device.DeviceSquares(k, 1, ctx=ctx)
    sq.load_ods(np.ascontiguousarray(ods).reshape(1, -1))
    sq.extend()
    torch.cuda.synchronize()
    assert int(sq.status[0]) == 0
    eds = sq.eds[0]
    cacher = inclusion.EDSSubTreeRootCacher(k, eds, ctx)
    cells = [(r, c) for r in range(w) for c in range(w)]
    proofs = proof.prove_row_ranges(cacher, [(r, c, c + 1) for r, c in cells])
    nss, ns_ix = [b"\xff" * 29], {b"\xff" * 29: 0}
    desc = np.zeros((len(cells), 8), np.int64)
    nodes = []
    for i, ((r, c), p) in enumerate(zip(cells, proofs)):
        ns = bytes(ods[r * k + c][:29]) if r < k and c < k else b"\xff" * 29
        if ns not in ns_ix:
            ns_ix[ns] = len(nss)
            nss.append(ns)
        desc[i] = (c, c + 1, 1, r * w + c, len(p.nodes), len(nodes), ns_ix[ns], r)
        nodes.extend(p.nodes)
    dev = eds.device
    t_ns = torch.from_numpy(np.frombuffer(b"".join(nss), np.uint8).copy()).to(dev)
    t_nodes = torch.from_numpy(np.frombuffer(b"".join(nodes), np.uint8).copy()).to(dev)
    roots = sq.row_roots[0].reshape(-1)
    st = device.nmt_verify_batch_device(desc, t_ns, eds, 512, t_nodes, roots, ctx=ctx)
    assert st.dtype == torch.int32 and st.is_cuda
    assert (st.cpu().numpy() == OK).all()
    victim = 5 * w + 19  # a parity cell
    eds[victim * 512 + 300] ^= 1
    st = device.nmt_verify_batch_device(desc, t_ns, eds, 512, t_nodes, roots, ctx=ctx).cpu().numpy()
    assert st[victim] == ERR_PROOF and (np.delete(st, victim) == OK).all()


# ---- validate_batch end to end -----------------------------------------------------------

def test_validate_batch_equals_validate(ctx):
    from dataclasses import replace
    k = 8
    # two namespaces of 32 shares each, so that the ranges below hold one namespace
    s = np.random.default_rng(8).integers(0, 256, size=(k * k, 512), dtype=np.uint8)
    s[:, :19] = 0
    s[:32, 19:29] = 0x11
    s[32:, 19:29] = 0x22
    ods = synth.sort_shares(s)
    shares = [ods[i].tobytes() for i in range(k * k)]
    data_root = da.new_data_availability_header(da.extend_shares(ods, ctx)).hash()
    proofs, roots = [], []
    for start, end in ((10, 11), (17, 22), (5, 23)):  # one share, inside one row, three rows
        sp = proof.new_share_inclusion_proof(shares, shares[start][:29], (start, end), ctx)
        assert len(sp.share_proofs) == (end - 1) // k - start // k + 1
        bad_data = list(sp.data)
        bad_data[-1] = bad_data[-1][:300] + bytes([bad_data[-1][300] ^ 4]) + bad_data[-1][301:]
        rp = sp.row_proof
        bad_root = bytes([rp.row_roots[0][60] ^ 1])
        bad_roots = [rp.row_roots[0][:60] + bad_root + rp.row_roots[0][61:]] + rp.row_roots[1:]
        mp = rp.proofs[-1]
        bad_mp = rp.proofs[:-1] + [proof.MerkleProof(mp.total, mp.index, mp.leaf_hash,
                                                     [bytes([mp.aunts[0][0] ^ 1]) + mp.aunts[0][1:]] + mp.aunts[1:])]
        variants = [
            (sp, data_root),
            (replace(sp, data=bad_data), data_root),                                   # a tampered data share
            (replace(sp, row_proof=replace(rp, row_roots=bad_roots)), data_root),      # a tampered row root
            (replace(sp, row_proof=replace(rp, proofs=bad_mp)), data_root),            # a tampered aunt
            (sp, hashlib.sha256(data_root).digest()),                                  # a wrong data root
            (replace(sp, share_proofs=sp.share_proofs + [sp.share_proofs[-1]]), data_root),  # count mismatch
        ]
        for p, r in variants:
            proofs.append(p)
            roots.append(r)
    want = []
    for p, r in zip(proofs, roots):
        try:
            p.validate(r)
            want.append(None)
        except da.DAError as e:
            want.append((e.code, str(e)))
    got = proof.validate_batch(proofs, roots, ctx)
    assert [None if g is None else (g.code, str(g)) for g in got] == want
    assert want[0] is None and want[6] is None and want[12] is None
    assert sum(w is None for w in want) == 3
    # one data root for the whole list
    same = [p for p, r in zip(proofs, roots) if r == data_root]
    got = proof.validate_batch(same, data_root, ctx)
    assert [g is None for g in got] == [w is None for w, r in zip(want, roots) if r == data_root]
