"""Namespace proofs from a resident square and their batched verification
(dagpu_nmt_namespace_ranges_device, dagpu_nmt_prove_namespace_batch_device,
dagpu_nmt_verify_namespace_batch(_device); device.nmt_*namespace*,
proof.prove_namespaces / verify_namespace_data).

The specification is the Python model of the rules in include/dagpu.h over the
oracle's pure-Python nmt hasher (tests/nmt_namespace_model.py) and, for the
verifier's statuses, the library's host verifier dagpu_nmt_verify_namespace,
itself checked against the model in tests/test_nmt_namespace_host.py."""
import ctypes
import random

import numpy as np
import pytest
import torch

import nmt_namespace_model as model
from celestia_da import _abi, da, device, inclusion, proof

pytestmark = pytest.mark.gpu

OK, ERR_PROOF, ERR_ARG = _abi.OK, _abi.ERR_PROOF, _abi.ERR_ARG
SEEDS = {1: 40, 2: 55, 4: 40, 8: 8}  # k = 2, 4: seeds whose runs leave a namespace absent inside a row


@pytest.fixture(scope="module")
def ctx():
    c = da.Context(0)
    yield c
    c.close()


def _popcount(v):
    return bin(int(v)).count("1")


class NsSquare:
    """One test square on the device with its row store; for the small widths
    every row tree rebuilt with pyref and the model's answer to every query."""

    def __init__(self, ctx, k, seed, runs=None, reference=True):
        self.k, self.w = k, 2 * k
        w = self.w
        self.runs = runs or model.run_lengths(k, seed)
        self.ods = model.namespaced_square(k, seed, self.runs)
        self.sq = device.DeviceSquares(k, 1, ctx=ctx)
        self.sq.load_ods(np.ascontiguousarray(self.ods).reshape(1, -1))
        self.sq.extend()
        torch.cuda.synchronize()
        # row-major sorted namespaces: every row and column is in push order
        assert int(self.sq.status[0]) == 0
        self.nodes = inclusion.EDSAxisNodes(k, self.sq.eds[0], ctx)
        self.d_roots = self.sq.row_roots[0].reshape(-1).contiguous()
        self.row_roots = [r.tobytes() for r in self.sq.row_roots[0].cpu().numpy()]
        if not reference:
            return
        self.qs = model.queries(len(self.runs))
        self.eds = self.sq.eds[0].cpu().numpy().reshape(w * w, 512)
        self.cells = [[self.eds[r * w + c].tobytes() for c in range(w)] for r in range(w)]
        ns = model.row_namespaces(self.ods, k)
        self.trees = [model.Tree([model.pyref.leaf(ns[r][c], self.cells[r][c]) for c in range(w)]) for r in range(w)]
        assert [t.root for t in self.trees] == self.row_roots
        self.want = model.model_ranges(self.ods, k, self.qs)
        # the proofs with kind != 0 in (query, row) order
        self.proofs = [(q, r) + model.prove_namespace(self.trees[r], self.qs[q])
                       for q in range(len(self.qs)) for r in range(w) if self.want[q, r, 0] != model.OUTSIDE]


_squares = {}


def _square(ctx, k):
    if k not in _squares:
        _squares[k] = NsSquare(ctx, k, SEEDS[k])
    return _squares[k]


def _counts(want, m):
    """counts_out from the model's ranges: proofs, absent, proof nodes, proven cells."""
    hit = want[want[:, :, 0] != model.OUTSIDE]
    return [len(hit), int((hit[:, 0] == model.ABSENT).sum()),
            sum(_popcount(s) + m - _popcount(e - 1) for _, s, e in hit),
            int((hit[hit[:, 0] == model.PRESENT][:, 2] - hit[hit[:, 0] == model.PRESENT][:, 1]).sum())]


def host_verify(nid, leaves, start, end, nodes, leaf_hash, root):
    p = proof.NMTProof(start, end, list(nodes), leaf_hash)
    return OK if p.verify_namespace(nid, [nid + x for x in leaves], root) else ERR_PROOF


# ---- search ------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_ranges(ctx, k):
    s = _square(ctx, k)
    ranges, counts = device.nmt_namespace_ranges_device(s.nodes, s.qs, ctx=ctx)
    assert ranges.shape == s.want.shape and (ranges == s.want).all(), np.argwhere(ranges != s.want)[:4]
    assert counts.tolist() == _counts(s.want, s.w.bit_length() - 1)
    kind = ranges[:, :, 0]
    assert (kind == model.PRESENT).any() and (kind == model.OUTSIDE).any()
    assert k == 1 or (kind == model.ABSENT).any()
    if k == 8:
        assert len(s.qs) == 26
        assert ((kind == 0).sum(), (kind == 1).sum(), (kind == 2).sum()) == (388, 22, 6)
        present = ranges[kind == 1]
        assert ((present[:, 1] == 0) & (present[:, 2] == 16)).sum() == 8      # the parity rows, whole
        assert ((present[:, 1] == 0) & (present[:, 2] == 8)).sum() == 3       # whole Q0 halves
        assert (present[:, 1] == 0).sum() == 16 and (present[:, 2] == 8).sum() == 8


# ---- production --------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_proofs(ctx, k):
    s = _square(ctx, k)
    nodes, ns, shares, hashes, desc, pairs, counts = device.nmt_prove_namespace_batch_device(s.nodes, s.qs, ctx=ctx)
    torch.cuda.synchronize()
    nodes, ns, hashes = (t.cpu().numpy().tobytes() for t in (nodes, ns, hashes))
    shares = shares.cpu().numpy().reshape(-1, 512)
    assert ns == b"".join(s.qs)
    assert counts.tolist() == _counts(s.want, s.w.bit_length() - 1)
    assert len(desc) == len(pairs) == len(s.proofs) == counts[0]
    node_off = leaf_off = n_abs = 0
    for i, (q, r, kind, a, b, want_nodes, want_lh) in enumerate(s.proofs):
        absent = kind == model.ABSENT
        assert pairs[i].tolist() == [q, r]
        assert desc[i].tolist() == [a, b, 0 if absent else b - a, leaf_off, len(want_nodes), node_off, q, r,
                                    n_abs if absent else -1], (q, r)
        assert nodes[90 * node_off:90 * (node_off + len(want_nodes))] == b"".join(want_nodes), (q, r)
        if absent:
            assert hashes[90 * n_abs:90 * (n_abs + 1)] == want_lh == s.trees[r].leaves[a], (q, r)
            n_abs += 1
        else:
            assert (shares[leaf_off:leaf_off + b - a] == s.eds[r * s.w + a:r * s.w + b]).all(), (q, r)
            leaf_off += b - a
        node_off += len(want_nodes)
    assert (len(nodes), len(shares), len(hashes)) == (90 * node_off, leaf_off, 90 * n_abs)
    # the convenience form: per namespace (row, proof, shares)
    got = proof.prove_namespaces(s.nodes, s.qs)
    flat = [(q, row, p.start, p.end, p.nodes, p.leaf_hash) for q, rows in enumerate(got) for row, p, _ in rows]
    assert flat == [(q, r, a, b, n, lh) for q, r, _, a, b, n, lh in s.proofs]
    for q, rows in enumerate(got):
        for row, p, sh in rows:
            assert sh == (s.cells[row][p.start:p.end] if not p.is_of_absence() else [])


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_round_trip_on_one_stream(ctx, k):
    s = _square(ctx, k)
    nodes, ns, shares, hashes, desc, pairs, _ = device.nmt_prove_namespace_batch_device(s.nodes, s.qs, ctx=ctx)
    st = device.nmt_verify_namespace_batch_device(desc, ns, shares, 512, nodes, hashes, s.d_roots, ctx=ctx)
    assert st.is_cuda
    st = st.cpu().numpy()
    assert len(st) == len(s.proofs) and (st == OK).all(), np.nonzero(st != OK)[0][:8]
    for q, r, kind, a, b, pn, lh in s.proofs:
        lv = s.cells[r][a:b] if kind == model.PRESENT else []
        assert host_verify(s.qs[q], lv, a, b, pn, lh, s.row_roots[r]) == OK, (q, r)
    # presence proofs may read their shares from the square itself
    rows = np.array([i for i, p in enumerate(s.proofs) if p[2] == model.PRESENT])
    d2 = desc.copy()
    d2[rows, 3] = [s.proofs[i][1] * s.w + s.proofs[i][3] for i in rows]
    st = device.nmt_verify_namespace_batch_device(d2, ns, s.nodes.eds, 512, nodes, hashes, s.d_roots, ctx=ctx)
    assert (st.cpu().numpy() == OK).all()


# ---- the verifier equals its specification -----------------------------------------------

_pool = {}


def _proof_pool(ctx):
    """(class, nid, leaves, start, end, nodes, leaf_hash, root) of the k = 8 square:
    every valid proof (the empty ones of some outside pairs included) and every
    tamper of each, with the host verifier's status."""
    if "items" not in _pool:
        s = _square(ctx, 8)
        items = []
        for q, nid in enumerate(s.qs):
            for r in range(s.w):
                kind, a, b, pn, lh = model.prove_namespace(s.trees[r], nid)
                if kind == model.OUTSIDE and (q + r) % 7:
                    continue
                lv = s.cells[r][a:b] if kind == model.PRESENT else []
                items.append(("valid", nid, lv, a, b, pn, lh, s.row_roots[r]))
                for name, (tl, ts, te, tn, th, tr) in model.tampers(s.trees[r], s.cells[r], nid, kind, a, b, pn, lh):
                    items.append((name, nid, tl, ts, te, tn, th, tr))
        _pool["items"] = items
        _pool["host"] = np.array([host_verify(*it[1:]) for it in items], np.int32)
    return _pool["items"], _pool["host"]


def _pack(items):
    return proof.pack_namespace_proofs([(proof.NMTProof(a, b, list(pn), lh), nid, lv, root)
                                        for _, nid, lv, a, b, pn, lh, root in items], 512)


def _dev(b, dev="cuda"):
    return torch.from_numpy(np.frombuffer(b, np.uint8).copy()).to(dev) if len(b) else \
        torch.empty(0, dtype=torch.uint8, device=dev)


def _device_form(pk, ctx):
    st = device.nmt_verify_namespace_batch_device(pk.desc, _dev(pk.namespaces), _dev(pk.leaves), 512, _dev(pk.nodes),
                                                  _dev(pk.leaf_hashes), _dev(pk.roots), ctx=ctx)
    return st.cpu().numpy()


def test_verifier_equals_host_verifier(ctx):
    items, host = _proof_pool(ctx)
    classes = {it[0] for it in items}
    assert classes == {"valid", "drop_first", "drop_last", "empty_for_present", "empty_for_absent", "absent_right",
                       "absent_left", "absent_with_leaves", "present_with_leaf_hash", "flipped_byte", "wrong_root",
                       "node_removed", "empty_with_leaves"}
    for it, h in zip(items, host):
        assert (h == OK) == (it[0] == "valid"), it[0]
    valid = [it for it in items if it[0] == "valid"]
    assert any(it[3] == it[4] for it in valid) and any(it[6] for it in valid) and any(it[2] for it in valid)
    pk = _pack(items)
    assert pk.desc.shape[1] == 9 and pk.n_leaf_hashes > 0
    st_host_form = proof._run_namespace(pk, ctx)
    assert (st_host_form == host).all(), [items[i][0] for i in np.nonzero(st_host_form != host)[0][:8]]
    st_dev = _device_form(pk, ctx)
    assert (st_dev == host).all(), [items[i][0] for i in np.nonzero(st_dev != host)[0][:8]]
    # the Python mirror: prefixed leaves, bools
    some = items[::5]
    got = proof.verify_namespace_batch([(proof.NMTProof(a, b, list(pn), lh), nid, [nid + x for x in lv], root)
                                        for _, nid, lv, a, b, pn, lh, root in some], ctx)
    assert got == [bool(h == OK) for h in host[::5]]


@pytest.mark.parametrize("n", [65, 129])
def test_divergent_lanes(ctx, n):
    items, host = _proof_pool(ctx)
    rng = random.Random(n)
    # one wave mixes empty, absence and presence proofs of 1 .. 2k leaves
    special = [i for i, it in enumerate(items) if it[0] == "valid" and len(it[2]) == 16][:2]
    special += [i for i, it in enumerate(items) if it[0] == "valid" and it[3] == it[4]][:1]
    special += [i for i, it in enumerate(items) if it[0] == "valid" and it[6]][:1]
    special += [i for i, it in enumerate(items) if it[0] == "valid" and len(it[2]) == 1][:1]
    assert len(special) == 5
    pick = rng.sample([i for i in range(len(items)) if i not in special], n - 5)
    for i in special:  # into the first wave, at shuffled lanes
        pick.insert(rng.randrange(60), i)
    assert len(pick) == n
    sub = [items[i] for i in pick]
    first = sub[:64]
    assert any(it[0] == "valid" and it[3] == it[4] for it in first) and any(it[0] == "valid" and it[6] for it in first)
    assert {0, 1, 16} <= {len(it[2]) for it in first}
    pk = _pack(sub)
    want = host[pick]
    assert (_device_form(pk, ctx) == want).all() and (proof._run_namespace(pk, ctx) == want).all()
    assert (want == OK).any() and (want == ERR_PROOF).any()


# ---- workload width ----------------------------------------------------------------------

def test_workload_width(ctx):
    k, w = 128, 256
    runs = [100, 400, 28, k * k - 528]
    s = NsSquare(ctx, k, 128, runs=runs, reference=False)
    ids = [model.ns_id(v) for v in (16, 18, 20, 22, 17, 19, 15)] + [model.PARITY]
    # 18 spans rows 0 .. 3; 17 and 19 are absent inside rows 0 and 3; 15 is outside every row
    nodes, ns, shares, hashes, desc, pairs, counts = device.nmt_prove_namespace_batch_device(s.nodes, ids, ctx=ctx)
    st = device.nmt_verify_namespace_batch_device(desc, ns, shares, 512, nodes, hashes, s.d_roots, ctx=ctx)
    st = st.cpu().numpy()
    assert (st == OK).all(), np.nonzero(st != OK)[0][:8]
    # numpy recomputation from the row roots and the Q0 namespaces
    roots = np.frombuffer(b"".join(s.row_roots), np.uint8).reshape(w, 90)
    rmin, rmax = [r[:29].tobytes() for r in roots], [r[29:58].tobytes() for r in roots]
    inside = np.array([[rmin[r] <= nid <= rmax[r] for r in range(w)] for nid in ids])
    assert len(desc) == counts[0] == inside.sum()
    assert [tuple(p) for p in pairs] == [(q, r) for q in range(len(ids)) for r in range(w) if inside[q, r]]
    q0 = s.ods[:, :29].reshape(k, k, 29)
    have = np.array([[(q0[r] == np.frombuffer(nid, np.uint8)).all(axis=1).sum() if r < k else
                      (w if nid == model.PARITY else 0) for r in range(w)] for nid in ids])
    assert counts[3] == have.sum() and counts[1] == (inside & (have == 0)).sum() == 2
    assert inside[1].sum() == 4 and inside[6].sum() == 0 and inside[7].sum() == k
    per_proof = [have[q, r] for q, r in pairs]
    assert desc[:, 2].tolist() == per_proof and (desc[:, 1] - desc[:, 0]).tolist() == [max(c, 1) for c in per_proof]
    # the light client's whole check, from the host-side form
    got = proof.prove_namespaces(s.nodes, ids[:7])
    for q in (1, 4, 5, 6):
        assert len(got[q]) == inside[q].sum()
        assert proof.verify_namespace_data(s.row_roots, ids[q], got[q], ctx)
    assert not proof.verify_namespace_data(s.row_roots, ids[1], got[1][:2] + got[1][3:], ctx)
    assert not proof.verify_namespace_data(s.row_roots, ids[4], [], ctx)
    assert not proof.verify_namespace_data(s.row_roots, ids[1], got[0], ctx)


# ---- arguments ---------------------------------------------------------------------------

def test_capacities_and_empty_batch(ctx):
    k = 4
    s = _square(ctx, k)
    L = ctx._L
    dev = s.nodes.nodes.device
    q = np.frombuffer(b"".join(s.qs), np.uint8).reshape(-1, 29).copy()
    need = _counts(s.want, s.w.bit_length() - 1)  # proofs, absent, nodes, cells
    assert all(v > 0 for v in need)
    fill, word = 0xA5, -0x5A5A5A5A5A5A5A5B
    ws = torch.empty(L.dagpu_nmt_namespace_workspace_size(k, len(q)), dtype=torch.uint8, device=dev)

    def call(n_q, proofs, absent, nodes, cells):
        out_nodes = torch.full((90 * need[2] + 90,), fill, dtype=torch.uint8, device=dev)
        out_ns = torch.full((29 * len(q),), fill, dtype=torch.uint8, device=dev)
        out_sh = torch.full((512 * need[3] + 512,), fill, dtype=torch.uint8, device=dev)
        out_lh = torch.full((90 * need[1] + 90,), fill, dtype=torch.uint8, device=dev)
        desc = np.full((need[0] + 1, 9), word, np.int64)
        pairs = np.full((need[0] + 1, 2), 0x5A5A5A5A, np.int32)
        counts = np.full(4, word, np.int64)
        rc = L.dagpu_nmt_prove_namespace_batch_device(
            ctx.handle, k, n_q, q.ctypes.data, s.nodes.eds.data_ptr(), s.nodes.nodes.data_ptr(),
            out_nodes.data_ptr(), nodes, out_ns.data_ptr(), out_sh.data_ptr(), cells, out_lh.data_ptr(), absent,
            desc.ctypes.data, pairs.ctypes.data, proofs, counts.ctypes.data, ws.data_ptr(),
            torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        untouched = all(bool((t == fill).all()) for t in (out_nodes, out_ns, out_sh, out_lh)) and \
            bool((desc == word).all()) and bool((pairs == 0x5A5A5A5A).all())
        return rc, untouched, counts.tolist(), (out_nodes, out_sh, out_lh, desc)

    rc, untouched, counts, (out_nodes, out_sh, out_lh, desc) = call(len(q), need[0], need[1], need[2], need[3])
    assert rc == OK and not untouched and counts == need
    # exact capacities: the spare entries behind them stay as they were
    assert bool((out_nodes[90 * need[2]:] == fill).all()) and bool((out_sh[512 * need[3]:] == fill).all())
    assert bool((out_lh[90 * need[1]:] == fill).all()) and bool((desc[need[0]:] == word).all())
    for short in range(4):
        caps = list(need)
        caps[short] -= 1
        rc, untouched, counts, _ = call(len(q), *caps)
        assert rc == ERR_ARG and untouched and counts == need, short
        assert "capacity" in ctx.last_error()
    rc, untouched, counts, _ = call(0, 0, 0, 0, 0)
    assert rc == OK and untouched and counts == [0, 0, 0, 0]
    ranges, cnt = device.nmt_namespace_ranges_device(s.nodes, [], ctx=ctx)
    assert ranges.shape == (0, s.w, 3) and cnt.tolist() == [0, 0, 0, 0]
    assert proof.prove_namespaces(s.nodes, []) == []
    with pytest.raises(da.DAError) as e:
        device.nmt_prove_namespace_batch_device(s.nodes, s.qs, caps=(need[0], need[2] - 1, need[3], need[1]), ctx=ctx)
    assert e.value.code == ERR_ARG


def test_bad_descriptor_fails_the_call_and_leaves_status(ctx):
    s = _square(ctx, 4)
    L = ctx._L
    items = [("valid", s.qs[q], s.cells[r][a:b] if kind == model.PRESENT else [], a, b, pn, lh, s.row_roots[r])
             for q, r, kind, a, b, pn, lh in s.proofs]
    pk = _pack(items)
    assert pk.n_leaf_hashes >= 1
    absent = int(np.nonzero(pk.desc[:, 8] >= 0)[0][0])
    tensors = [_dev(x) for x in (pk.namespaces, pk.leaves, pk.nodes, pk.leaf_hashes, pk.roots)]
    ws = torch.empty(L.dagpu_nmt_verify_namespace_workspace_size(len(items), pk.n_leaves), dtype=torch.uint8,
                     device="cuda")
    for at, word, bad in ((absent, 8, pk.n_leaf_hashes), (0, 8, -2), (1, 8, 1 << 40), (0, 6, pk.n_ns),
                          (0, 7, -1), (1, 5, pk.n_nodes + 1)):
        d = pk.desc.copy()
        d[at, word] = bad
        status = torch.full((len(items),), 77, dtype=torch.int32, device="cuda")
        rc = L.dagpu_nmt_verify_namespace_batch_device(
            ctx.handle, len(items), d.ctypes.data, tensors[0].data_ptr(), pk.n_ns, tensors[1].data_ptr(),
            pk.n_leaves, 512, tensors[2].data_ptr(), pk.n_nodes, tensors[3].data_ptr(), pk.n_leaf_hashes,
            tensors[4].data_ptr(), pk.n_roots, status.data_ptr(), ws.data_ptr(),
            torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == ERR_ARG and bool((status == 77).all()), (at, word, bad)
        host_status = np.full(len(items), 77, np.int32)
        bufs = [np.frombuffer(x, np.uint8) for x in (pk.namespaces, pk.leaves, pk.nodes, pk.leaf_hashes, pk.roots)]
        rc = L.dagpu_nmt_verify_namespace_batch(
            ctx.handle, len(items), d.ctypes.data, bufs[0].ctypes.data, pk.n_ns, bufs[1].ctypes.data, pk.n_leaves,
            512, bufs[2].ctypes.data, pk.n_nodes, bufs[3].ctypes.data, pk.n_leaf_hashes, bufs[4].ctypes.data,
            pk.n_roots, host_status.ctypes.data)
        assert rc == ERR_ARG and (host_status == 77).all(), (at, word, bad)
    # and the same buffers verify when nothing is wrong
    assert (_device_form(pk, ctx) == OK).all()
