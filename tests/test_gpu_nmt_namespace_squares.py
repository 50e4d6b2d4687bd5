"""Namespace proofs across the squares of a batch proof store, on to the data
root (dagpu_nmt_namespace_squares_count_device,
dagpu_nmt_prove_namespace_squares_device; device.nmt_*namespace_squares*,
proof.prove_namespaces_squares, DeviceSquares.namespace_proofs).

The specification is the single-square call dagpu_nmt_prove_namespace_batch_device
on the slices of every square, regrouped into (query, square, row) order, and
for the small batches the Python model of the rules in include/dagpu.h
(tests/nmt_namespace_model.py) on trees rebuilt with the oracle's hasher.

Squares: model.namespaced_square.  Square 0 of width k has the seed and the runs
of tests/test_gpu_nmt_namespace.py; square i > 0 has seed + i (k = 8, whose runs
the model fixes, draws them from the seed as the other widths do).  At k = 1 a
square is one share, so every square has the one namespace 16: the property "a
namespace present in one square and not in another" needs k >= 2, as an
absence proof does."""
import random

import numpy as np
import pytest
import torch

import nmt_namespace_model as model
from celestia_da import _abi, da, device, proof

pytestmark = pytest.mark.gpu

OK, ERR_PROOF, ERR_ARG = _abi.OK, _abi.ERR_PROOF, _abi.ERR_ARG
SEEDS = {1: 40, 2: 55, 4: 40, 8: 8}  # tests/test_gpu_nmt_namespace.py


@pytest.fixture(scope="module")
def ctx():
    c = da.Context(0)
    yield c
    c.close()


def _popcount(v):
    return bin(int(v)).count("1")


def _runs(k, i):
    seed = SEEDS[k] + i
    if i == 0 or k != 8:
        return model.run_lengths(k, seed)
    rng, runs, left = random.Random(seed), [], k * k
    while left:
        r = min(rng.randint(1, 2 * k), left)
        runs.append(r)
        left -= r
    return runs


def _union(lists):
    out = []
    for qs in lists:
        out += [q for q in qs if q not in out]
    return out


class Batch:
    """n test squares of width k, extended in one DeviceSquares, with the model's
    answer to every (query, square, row); with reference=True every row tree is
    rebuilt with pyref.  strided(): the same squares 4096 B apart."""

    def __init__(self, ctx, k, n, reference=True):
        self.ctx, self.k, self.w, self.n = ctx, k, 2 * k, n
        w = self.w
        self.runs = [_runs(k, i) for i in range(n)]
        self.ods = [model.namespaced_square(k, SEEDS[k] + i, self.runs[i]) for i in range(n)]
        self.sq = device.DeviceSquares(k, n, ctx=ctx)
        self.sq.load_ods(np.stack([np.ascontiguousarray(o).reshape(-1) for o in self.ods]))
        self.sq.extend()
        torch.cuda.synchronize()
        assert (self.sq.status.cpu().numpy() == 0).all()
        self.store = self.sq.proof_store()
        self.row_roots = [[r.tobytes() for r in sq] for sq in self.sq.row_roots.cpu().numpy()]
        self.qs = _union(model.queries(len(r)) for r in self.runs)
        self.qs.append(self.qs[2])  # one duplicate: namespace 16, present in every square
        self._strided = None
        if not reference:
            return
        self.want = np.stack([model.model_ranges(o, k, self.qs) for o in self.ods], axis=1)  # (q, square, row, 3)
        eds = self.sq.eds.cpu().numpy().reshape(n, w * w, 512)
        self.cells = [[[eds[i, r * w + c].tobytes() for c in range(w)] for r in range(w)] for i in range(n)]
        self.trees = []
        for i in range(n):
            ns = model.row_namespaces(self.ods[i], k)
            self.trees.append([model.Tree([model.pyref.leaf(ns[r][c], self.cells[i][r][c]) for c in range(w)])
                               for r in range(w)])
            assert [t.root for t in self.trees[i]] == self.row_roots[i]
        # the batch has what the tests are about
        kind = self.want[..., 0]
        assert (kind == model.PRESENT).any() and (kind == model.OUTSIDE).any()
        if k >= 2:
            assert (kind == model.ABSENT).any()
        if k >= 2 and n >= 2:
            here = (kind == model.PRESENT).any(axis=2)  # (q, square)
            assert (here.any(axis=1) & ~here.all(axis=1)).any()
        # the proofs with kind != 0 in (query, square, row) order
        self.proofs = [(q, i, r) + model.prove_namespace(self.trees[i][r], self.qs[q])
                       for q in range(len(self.qs)) for i in range(n) for r in range(w)
                       if kind[q, i, r] != model.OUTSIDE]

    def strided(self):
        if self._strided is None:
            one = self.w * self.w * 512
            stride = one + 4096
            buf = torch.full((self.n * stride,), 0xEE, dtype=torch.uint8, device=self.sq.eds.device)
            buf.view(self.n, stride)[:, :one] = self.sq.eds
            self._strided = device.ProofStore(self.k, buf, square_stride=stride, ctx=self.ctx)
            assert self._strided.n == self.n
        return self._strided


_batches = {}


def _batch(ctx, k, n):
    if (k, n) not in _batches:
        _batches[k, n] = Batch(ctx, k, n)
    return _batches[k, n]


def _single_calls(store, qs, ctx):
    """What the loop of single-square calls gives, regrouped: the proofs in
    (query, square, row) order as (q, square, row, desc9, nodes, shares,
    leaf_hash), and the per-square counts."""
    out, counts = [], []
    for i in range(store.n):
        nodes, _, shares, hashes, desc, pairs, cnt = device.nmt_prove_namespace_batch_device(store.square(i), qs,
                                                                                               ctx=ctx)
        nodes, shares, hashes = (t.cpu().numpy().tobytes() for t in (nodes, shares, hashes))
        counts.append(cnt)
        for d, (q, row) in zip(desc.tolist(), pairs.tolist()):
            out.append((q, i, row, d, nodes[90 * d[5]:90 * (d[5] + d[4])], shares[512 * d[3]:512 * (d[3] + d[2])],
                        hashes[90 * d[8]:90 * d[8] + 90] if d[8] >= 0 else b""))
    out.sort(key=lambda p: p[:3])
    return out, np.array(counts)


def _host(r):
    """The device outputs of one produce call as bytes."""
    torch.cuda.synchronize()
    return {name: getattr(r, name).cpu().numpy().tobytes()
            for name in ("nodes", "namespaces", "shares", "leaf_hashes", "axis_roots", "dah_leaf_hashes", "aunts")
            if getattr(r, name) is not None}


def _assert_equals_single(r, h, single, qs, la):
    """Every output of the produce call `r` (host bytes `h`) against the
    regrouped single-square proofs."""
    n = len(single)
    assert len(r.desc) == len(r.hits) == n == r.counts[0]
    assert h["namespaces"] == b"".join(qs)
    node_off = leaf_off = n_abs = 0
    want_desc, want_hits, nodes, shares, hashes = [], [], [], [], []
    for i, (q, sq, row, d, pn, sh, lh) in enumerate(single):
        absent = d[8] >= 0
        want_desc.append([d[0], d[1], d[2], leaf_off, d[4], node_off, q, i, n_abs if absent else -1])
        want_hits.append([q, sq, row, model.ABSENT if absent else model.PRESENT, d[0], d[1]])
        nodes.append(pn)
        shares.append(sh)
        hashes.append(lh)
        node_off, leaf_off, n_abs = node_off + d[4], leaf_off + d[2], n_abs + absent
    assert r.desc.tolist() == want_desc
    assert r.hits.tolist() == want_hits
    assert r.counts.tolist() == [n, n_abs, node_off, leaf_off]
    assert h["nodes"] == b"".join(nodes)
    assert h["shares"] == b"".join(shares)
    assert h["leaf_hashes"] == b"".join(hashes)
    if r.mdesc is not None:
        assert r.mdesc.tolist() == [[row, 1 << la, la, i * la, i, sq] for i, (_, sq, row, *_) in enumerate(single)]


def _per(proofs, n_q, n_sq):
    per = np.zeros((n_q, n_sq), np.int32)
    for p in proofs:
        per[p[0], p[1]] += 1
    return per


# ---- one square: the single-square call itself --------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_one_square_equals_the_single_square_call(ctx, k):
    b = _batch(ctx, k, 1)
    nodes, ns, shares, hashes, desc, pairs, counts = device.nmt_prove_namespace_batch_device(b.store.square(0), b.qs,
                                                                                             ctx=ctx)
    r = device.nmt_prove_namespace_squares_device(b.store, b.qs, ctx=ctx)
    h = _host(r)
    assert h["nodes"] == nodes.cpu().numpy().tobytes() and h["shares"] == shares.cpu().numpy().tobytes()
    assert h["leaf_hashes"] == hashes.cpu().numpy().tobytes() and h["namespaces"] == ns.cpu().numpy().tobytes()
    assert r.counts.tolist() == counts.tolist() and counts[0] > 0
    # the descriptors differ in root_index alone: the row there, the proof's own axis root here
    assert np.array_equal(np.delete(r.desc, 7, axis=1), np.delete(desc, 7, axis=1))
    assert r.desc[:, 7].tolist() == list(range(len(desc)))
    assert np.array_equal(r.hits[:, [0, 2]], pairs) and (r.hits[:, 1] == 0).all()
    assert np.array_equal(r.hits[:, 4:6], desc[:, 0:2])
    assert np.array_equal(r.hits[:, 3] == model.ABSENT, desc[:, 8] >= 0)
    assert h["axis_roots"] == b"".join(b.row_roots[0][row] for row in pairs[:, 1])


# ---- three squares: the single-square calls, the model, both strides ----------------------

@pytest.mark.parametrize("strided", [False, True], ids=["back_to_back", "stride_plus_4096"])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_three_squares(ctx, k, strided):
    b = _batch(ctx, k, 3)
    store = b.strided() if strided else b.store
    la = (4 * k).bit_length() - 1
    counts, per = device.nmt_namespace_squares_count_device(store, b.qs, ctx=ctx)
    r = device.nmt_prove_namespace_squares_device(store, b.qs, ctx=ctx)
    h = _host(r)
    single, single_counts = _single_calls(store, b.qs, ctx)
    _assert_equals_single(r, h, single, b.qs, la)
    assert counts.tolist() == r.counts.tolist() == single_counts.sum(axis=0).tolist()
    assert per.shape == (len(b.qs), 3) and np.array_equal(per, _per(single, len(b.qs), 3))
    assert per.sum(axis=0).tolist() == single_counts[:, 0].tolist()
    # and the model: ranges, nodes, leaf hashes, cells, the merkle half's leaves
    assert len(b.proofs) == len(single)
    m = b.w.bit_length() - 1
    assert r.counts.tolist() == [len(b.proofs), sum(p[3] == model.ABSENT for p in b.proofs),
                                 sum(_popcount(p[4]) + m - _popcount(p[5] - 1) for p in b.proofs),
                                 sum(p[5] - p[4] for p in b.proofs if p[3] == model.PRESENT)]
    for i, (q, sq, row, kind, a, e, want_nodes, want_lh) in enumerate(b.proofs):
        d = r.desc[i]
        assert r.hits[i].tolist() == [q, sq, row, kind, a, e], i
        assert h["nodes"][90 * d[5]:90 * (d[5] + d[4])] == b"".join(want_nodes), (q, sq, row)
        if kind == model.ABSENT:
            assert d[2] == 0 and h["leaf_hashes"][90 * d[8]:90 * d[8] + 90] == want_lh == b.trees[sq][row].leaves[a]
        else:
            assert d[8] == -1 and h["shares"][512 * d[3]:512 * (d[3] + d[2])] == b"".join(b.cells[sq][row][a:e])
        assert h["axis_roots"][90 * i:90 * i + 90] == b.row_roots[sq][row]


# ---- round trip on one stream -------------------------------------------------------------

def _merkle_status(ctx, r, h, aunts, data_roots, n_sq):
    n = len(r.mdesc)
    status = np.full(n, 77, np.int32)
    leaves, lh, au, roots = (np.frombuffer(x, np.uint8).copy() for x in (h["axis_roots"], h["dah_leaf_hashes"], aunts,
                                                                         data_roots))
    md = np.ascontiguousarray(r.mdesc)
    rc = ctx._L.dagpu_merkle_verify_batch(ctx.handle, n, md.ctypes.data, leaves.ctypes.data, n, 90, lh.ctypes.data,
                                          au.ctypes.data, len(au) // 32, roots.ctypes.data, n_sq,
                                          status.ctypes.data)
    assert rc == OK, ctx.last_error()
    return status


def _flip(t, at):
    t2 = t.clone()
    t2[at] ^= 1
    return t2


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_round_trip_on_one_stream(ctx, k):
    b = _batch(ctx, k, 3)
    r = device.nmt_prove_namespace_squares_device(b.store, b.qs, ctx=ctx)
    n = len(r.desc)

    def verify(nodes=r.nodes, shares=r.shares, hashes=r.leaf_hashes):
        st = device.nmt_verify_namespace_batch_device(r.desc, r.namespaces, shares, 512, nodes, hashes, r.axis_roots,
                                                      ctx=ctx)
        assert st.is_cuda
        return st.cpu().numpy()

    st = verify()  # no synchronisation between the produce call and this one
    assert len(st) == n and (st == OK).all(), np.nonzero(st != OK)[0][:8]
    h = _host(r)
    data_roots = b.store.data_roots().cpu().numpy().tobytes()
    assert data_roots == b.sq.dah.cpu().numpy().tobytes()  # what extend wrote
    mst = _merkle_status(ctx, r, h, h["aunts"], data_roots, 3)
    assert (mst == OK).all(), np.nonzero(mst != OK)[0][:8]

    def only(status, i):
        return status[i] != OK and (np.delete(status, i) == OK).all()

    # one flipped byte turns exactly its own proof bad
    i = int(np.nonzero(r.desc[:, 4] > 0)[0][-1])
    assert only(verify(nodes=_flip(r.nodes, 90 * int(r.desc[i, 5]) + 70)), i)
    present = np.nonzero(r.desc[:, 2] > 0)[0]
    i = int(present[len(present) // 2])
    assert only(verify(shares=_flip(r.shares, 512 * int(r.desc[i, 3]) + 100)), i)
    if k >= 2:
        i = int(np.nonzero(r.desc[:, 8] >= 0)[0][-1])
        assert only(verify(hashes=_flip(r.leaf_hashes, 90 * int(r.desc[i, 8]) + 70)), i)
    la = (4 * k).bit_length() - 1
    i = n // 2
    aunts = bytearray(h["aunts"])
    aunts[32 * (i * la + la - 1) + 5] ^= 1
    assert only(_merkle_status(ctx, r, h, bytes(aunts), data_roots, 3), i)
    # the host verifiers, proof by proof
    got = proof.prove_namespaces_squares(b.store, b.qs)
    seen = 0
    for q, per_square in enumerate(got):
        for sq, rows in enumerate(per_square):
            for row, p, shares, mp in rows:
                assert p.verify_namespace(b.qs[q], [b.qs[q] + x for x in shares], b.row_roots[sq][row]), (q, sq, row)
                mp.verify(data_roots[32 * sq:32 * sq + 32], b.row_roots[sq][row])
                assert (mp.total, mp.index, len(mp.aunts)) == (4 * k, row, la)
                seen += 1
    assert seen == n


# ---- scan boundaries ----------------------------------------------------------------------

def test_scan_boundaries_first_lane_last_lane_and_an_empty_block(ctx):
    k, w = 8, 16
    b = _batch(ctx, k, 3)
    # namespace 16 is in row 0 of square 0 (lane 0), the parity namespace in the last row of the last
    # square (the last lane); twelve queries below every row's range hit nothing in between
    qs = [model.ns_id(16)] + [model.ns_id(15)] * 12 + [model.PARITY]
    want = np.stack([model.model_ranges(o, k, qs) for o in b.ods], axis=1)
    hit = (want[..., 0] != model.OUTSIDE).reshape(-1)
    assert hit.size == 14 * 3 * 16 == 672 and hit.size % 256 != 0
    assert hit[0] and hit[-1]
    blocks = [hit[i:i + 256].any() for i in range(0, hit.size, 256)]
    assert blocks == [True, False, True]
    r = device.nmt_prove_namespace_squares_device(b.store, qs, ctx=ctx)
    h = _host(r)
    single, _ = _single_calls(b.store, qs, ctx)
    _assert_equals_single(r, h, single, qs, 5)
    lanes = (r.hits[:, 0].astype(np.int64) * 3 + r.hits[:, 1]) * w + r.hits[:, 2]
    assert lanes.tolist() == np.nonzero(hit)[0].tolist()
    st = device.nmt_verify_namespace_batch_device(r.desc, r.namespaces, r.shares, 512, r.nodes, r.leaf_hashes,
                                                  r.axis_roots, ctx=ctx)
    assert (st.cpu().numpy() == OK).all()


def test_scan_second_level_64_squares_257_queries(ctx):
    k, n_sq, n_q = 8, 64, 257
    b = Batch(ctx, k, n_sq, reference=False)
    fill = [model.ns_id(17 + 2 * (i % 13)) if i % 3 else model.ns_id(2000 + i) for i in range(n_q)]
    qs = (b.qs + fill)[:n_q - 1] + [model.PARITY]  # the last lane of the grid hits
    assert len(qs) == n_q and n_q * n_sq * 2 * k == 263168 > 1024 * 256
    counts, per = device.nmt_namespace_squares_count_device(b.store, qs, ctx=ctx)
    r = device.nmt_prove_namespace_squares_device(b.store, qs, caps=counts[[0, 2, 3, 1]], ctx=ctx)
    h = _host(r)
    single, single_counts = _single_calls(b.store, qs, ctx)
    _assert_equals_single(r, h, single, qs, 5)
    assert counts.tolist() == single_counts.sum(axis=0).tolist()
    assert np.array_equal(per, _per(single, n_q, n_sq))
    # hits in several chunks of 256 blocks, the last one included
    lanes = (r.hits[:, 0].astype(np.int64) * n_sq + r.hits[:, 1]) * 2 * k + r.hits[:, 2]
    assert (np.diff(lanes) > 0).all()
    assert len(np.unique(lanes >> 16)) >= 3 and lanes.max() >> 16 == (n_q * n_sq * 2 * k - 1) >> 16
    st = device.nmt_verify_namespace_batch_device(r.desc, r.namespaces, r.shares, 512, r.nodes, r.leaf_hashes,
                                                  r.axis_roots, ctx=ctx)
    assert (st.cpu().numpy() == OK).all()


# ---- proofs of more than log2(2k) nodes ---------------------------------------------------

def test_every_hit_has_more_than_log2_nodes(ctx):
    """A range astride a subtree boundary has up to 2 log2(2k) - 2 proof nodes: [3, 5) of 16 leaves has
    5.  One namespace whose only hit in each of three squares is such a two-share run (in rows 0, 1 and
    5), so the batch's node total is above proofs * log2(2k)."""
    k, w, m = 8, 16, 4
    nid = model.ns_id(18)  # run 1 of every square
    runs = [[3, 2, k * k - 5], [k + 3, 2, k * k - k - 5], [5 * k + 3, 2, k * k - 5 * k - 5]]
    ods = [model.namespaced_square(k, 300 + i, r) for i, r in enumerate(runs)]
    want = np.stack([model.model_ranges(o, k, [nid]) for o in ods], axis=1)[0]  # (square, row, 3)
    hit = want[want[..., 0] != model.OUTSIDE]
    assert hit.tolist() == [[model.PRESENT, 3, 5]] * 3
    assert np.argwhere(want[..., 0] != model.OUTSIDE).tolist() == [[0, 0], [1, 1], [2, 5]]
    assert _popcount(3) + m - _popcount(4) == 5 > m
    sq = device.DeviceSquares(k, 3, ctx=ctx)
    sq.load_ods(np.stack([np.ascontiguousarray(o).reshape(-1) for o in ods]))
    sq.extend()
    torch.cuda.synchronize()
    assert (sq.status.cpu().numpy() == 0).all()
    store = sq.proof_store()
    counts, per = device.nmt_namespace_squares_count_device(store, [nid], ctx=ctx)
    assert counts.tolist() == [3, 0, 15, 6] and per.tolist() == [[1, 1, 1]]
    r = device.nmt_prove_namespace_squares_device(store, [nid], ctx=ctx)
    h = _host(r)
    single, single_counts = _single_calls(store, [nid], ctx)
    _assert_equals_single(r, h, single, [nid], 5)
    assert r.counts.tolist() == single_counts.sum(axis=0).tolist() == [3, 0, 15, 6]
    assert r.hits.tolist() == [[0, 0, 0, 1, 3, 5], [0, 1, 1, 1, 3, 5], [0, 2, 5, 1, 3, 5]]
    assert r.desc[:, 4].tolist() == [5, 5, 5]
    st = device.nmt_verify_namespace_batch_device(r.desc, r.namespaces, r.shares, 512, r.nodes, r.leaf_hashes,
                                                  r.axis_roots, ctx=ctx)
    assert (st.cpu().numpy() == OK).all()
    roots = sq.row_roots.cpu().numpy()
    eds = sq.eds.cpu().numpy().reshape(3, w * w, 512)
    for i, (_, s_, row, _, a, e) in enumerate(r.hits.tolist()):
        p = proof.NMTProof(a, e, [h["nodes"][90 * j:90 * (j + 1)] for j in range(5 * i, 5 * i + 5)])
        assert p.verify_namespace(nid, [nid + eds[s_, row * w + c].tobytes() for c in range(a, e)],
                                  roots[s_, row].tobytes())


# ---- capacities and edge cases ------------------------------------------------------------

def test_capacities_and_edge_cases(ctx):
    k = 4
    b = _batch(ctx, k, 3)
    L, store = ctx._L, b.store
    dev = store.store.device
    q = np.frombuffer(b"".join(b.qs), np.uint8).reshape(-1, 29).copy()
    need = device.nmt_namespace_squares_count_device(store, b.qs, ctx=ctx)[0].tolist()  # proofs, absent, nodes, cells
    m, la = b.w.bit_length() - 1, (4 * k).bit_length() - 1
    assert need == [len(b.proofs), sum(p[3] == model.ABSENT for p in b.proofs),
                    sum(_popcount(p[4]) + m - _popcount(p[5] - 1) for p in b.proofs),
                    sum(p[5] - p[4] for p in b.proofs if p[3] == model.PRESENT)]
    assert all(v > 0 for v in need)
    fill, word, iword = 0xA5, -0x5A5A5A5A5A5A5A5B, 0x5A5A5A5A
    ws = torch.empty(L.dagpu_nmt_namespace_squares_workspace_size(k, 3, len(q), need[0]), dtype=torch.uint8,
                     device=dev)

    def call(n_q, proofs, absent, nodes, cells, n_sq=3, store_at=0, stride=store.square_stride, queries=q):
        dv = {name: torch.full((size + extra,), fill, dtype=torch.uint8, device=dev) for name, size, extra in
              (("nodes", 90 * need[2], 90), ("ns", 29 * len(q), 0), ("shares", 512 * need[3], 512),
               ("lh", 90 * need[1], 90), ("roots", 90 * need[0], 90), ("dlh", 32 * need[0], 32),
               ("aunts", 32 * la * need[0], 32))}
        desc = np.full((need[0] + 1, 9), word, np.int64)
        mdesc = np.full((need[0] + 1, 6), word, np.int64)
        hits = np.full((need[0] + 1, 6), iword, np.int32)
        counts = np.full(4, word, np.int64)
        rc = L.dagpu_nmt_prove_namespace_squares_device(
            ctx.handle, k, n_sq, n_q, queries.ctypes.data, store.eds.data_ptr(), stride,
            store.store.data_ptr() + store_at, dv["nodes"].data_ptr(), nodes, dv["ns"].data_ptr(),
            dv["shares"].data_ptr(), cells, dv["lh"].data_ptr(), absent, dv["roots"].data_ptr(),
            dv["dlh"].data_ptr(), dv["aunts"].data_ptr(), desc.ctypes.data, mdesc.ctypes.data, hits.ctypes.data,
            proofs, counts.ctypes.data, ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        device_untouched = {name: bool((t == fill).all()) for name, t in dv.items()}
        host_untouched = bool((desc == word).all()) and bool((mdesc == word).all()) and bool((hits == iword).all())
        return rc, device_untouched, host_untouched, counts.tolist(), (dv, desc, mdesc, hits)

    rc, dun, hun, counts, (dv, desc, mdesc, hits) = call(len(q), *need)
    assert rc == OK and not any(dun.values()) and not hun and counts == need
    # exact capacities: the spare entries behind them stay as they were
    for name, size in (("nodes", 90 * need[2]), ("shares", 512 * need[3]), ("lh", 90 * need[1]),
                       ("roots", 90 * need[0]), ("dlh", 32 * need[0]), ("aunts", 32 * la * need[0])):
        assert bool((dv[name][size:] == fill).all()), name
    assert (desc[need[0]:] == word).all() and (mdesc[need[0]:] == word).all() and (hits[need[0]:] == iword).all()
    assert hits[:need[0]].tolist() == [list(p[:6]) for p in b.proofs]
    for short in range(4):
        caps = list(need)
        caps[short] -= 1
        rc, dun, hun, counts, _ = call(len(q), *caps)
        assert rc == ERR_ARG and all(dun.values()) and hun and counts == need, short
        msg = ctx.last_error()
        assert "capacity" in msg and all(f"{what} {v}" in msg for what, v in
                                         zip(("proofs", "leaf hashes", "nodes", "cells"), need)), msg
    # no queries: accepted, nothing written
    rc, dun, hun, counts, _ = call(0, 0, 0, 0, 0)
    assert rc == OK and all(dun.values()) and hun and counts == [0, 0, 0, 0]
    cnt, per = device.nmt_namespace_squares_count_device(store, [], ctx=ctx)
    assert cnt.tolist() == [0, 0, 0, 0] and per.shape == (0, 3)
    assert proof.prove_namespaces_squares(store, []) == []
    # queries outside every row of every square: zero counts, only the query namespaces written
    outside = np.frombuffer(model.ns_id(15) + b"\x00" * 29 + b"\xff" * 28 + b"\xfe", np.uint8).reshape(3, 29).copy()
    rc, dun, hun, counts, (dv, *_) = call(3, 0, 0, 0, 0, queries=outside)
    assert rc == OK and hun and counts == [0, 0, 0, 0]
    assert all(v for name, v in dun.items() if name != "ns")
    assert dv["ns"][:87].cpu().numpy().tobytes() == outside.tobytes() and bool((dv["ns"][87:] == fill).all())
    r = device.nmt_prove_namespace_squares_device(store, [model.ns_id(15)], ctx=ctx)
    assert r.counts.tolist() == [0, 0, 0, 0] and len(r.desc) == len(r.hits) == r.nodes.numel() == 0
    cnt, per = device.nmt_namespace_squares_count_device(store, [model.ns_id(15)], ctx=ctx)
    assert cnt.tolist() == [0, 0, 0, 0] and per.tolist() == [[0, 0, 0]]
    # arguments
    for kwargs in ({"n_sq": 0}, {"store_at": 8}, {"stride": store.square_stride - 16}, {"stride": b.w * b.w * 512 + 8}):
        rc, dun, hun, counts, _ = call(len(q), *need, **kwargs)
        assert rc == ERR_ARG and all(dun.values()) and hun and counts == [word] * 4, kwargs
    assert L.dagpu_nmt_namespace_squares_count_device(ctx.handle, k, 0, len(q), q.ctypes.data, store.store.data_ptr(),
                                                      np.zeros(4, np.int64).ctypes.data, None, ws.data_ptr(),
                                                      torch.cuda.current_stream().cuda_stream) == ERR_ARG
    assert L.dagpu_nmt_namespace_squares_count_device(ctx.handle, 3, 3, len(q), q.ctypes.data, store.store.data_ptr(),
                                                      np.zeros(4, np.int64).ctypes.data, None, ws.data_ptr(),
                                                      torch.cuda.current_stream().cuda_stream) == ERR_ARG
    with pytest.raises(da.DAError) as e:
        device.nmt_prove_namespace_squares_device(store, b.qs, caps=(need[0], need[2] - 1, need[3], need[1]), ctx=ctx)
    assert e.value.code == ERR_ARG


# ---- convenience forms --------------------------------------------------------------------

@pytest.mark.parametrize("k", [2, 8])
def test_convenience_forms(ctx, k):
    b = _batch(ctx, k, 3)
    got = proof.prove_namespaces_squares(b.store, b.qs)
    assert len(got) == len(b.qs) and all(len(g) == 3 for g in got)
    per_square = [proof.prove_namespaces(b.store.square(i), b.qs) for i in range(3)]
    for q in range(len(b.qs)):
        for i in range(3):
            assert [(row, p, sh) for row, p, sh, _ in got[q][i]] == per_square[i][q], (q, i)
            assert proof.verify_namespace_data(b.row_roots[i], b.qs[q], [x[:3] for x in got[q][i]], ctx), (q, i)
    assert [(q, i, row, p.start, p.end, p.nodes, p.leaf_hash) for q, g in enumerate(got) for i, rows in enumerate(g)
            for row, p, _, _ in rows] == [(q, i, r, a, e, n, lh) for q, i, r, _, a, e, n, lh in b.proofs]
    assert b.sq.namespace_proofs(b.qs) == got
    # an answer with a row left out is refused
    q, i = next((q, i) for q in range(len(b.qs)) for i in range(3) if len(got[q][i]) >= 2)
    assert not proof.verify_namespace_data(b.row_roots[i], b.qs[q], [x[:3] for x in got[q][i][1:]], ctx)
