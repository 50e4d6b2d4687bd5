"""Every kernel that hashes, compares, packs or searches a namespace, on
namespaces that use all 29 bytes (tests/ns_corpus.py): the first differing byte
of neighbouring Q0 cells takes every position 0..28 on both axes, in row-major
and in column-major sorted squares, next to the 58 namespaces one bit away from
00*29 and FF*29 and to Q0 cells that carry the parity namespace itself.

 a  roots, DAH and status of DeviceSquares.extend (nmt.hip) against the oracle
 b  push order: the status bit of extend and the forest's check_order
 c  the forest on 512-B shares (nmt_forest.hip) and the node stores (proof_store.hip)
 d  range proofs (nmt_prove.hip) against nmt's buildRangeProof on pyref trees
 e  namespace search and proofs (nmt_namespace.hip), one square and a batch
 f  the batch verifiers (proof_verify.hip) against the host verifiers and the model
 g  one repair (repair.hip) and one byzantine report

Every comparison is bit-exact.  The references are the oracle (oracle/, C) for
squares and roots, and the Python model of nmt's proofs over pyref's hasher
(tests/nmt_namespace_model.py); tests/test_ns_corpus_host.py checks both, and
the host verifiers, on the same bytes without a GPU.

Out of scope: the blob-commitment and square-construction entry points validate
the namespace version (bytes 0..18 of a version-0 namespace are zero by rule),
so a full-width namespace never reaches their kernels.

What is compared (every figure a bit-exact comparison):
 a  45 squares in 15 batches of three at k = 1 .. 32 and two at k = 128: EDS,
    3208 row and column roots, DAH, status; 14 squares through the host entry
 b  146 violating squares (first differing byte 0, 7, 13, 24, 27, 28; three
    position classes; both axes; both layouts; FF*29 before a smaller cell), each
    in the three slots of a batch; 14 valid squares; the status of 11680 forest
    trees, raw shares and namespaced pushes
 c  384 wrapper roots of 8 squares; 2928 node records of 3 squares
 d  13056 range proofs at k = 8 (every range of every tree of 3 squares), 2048 at k = 32
 e  4961 queries on 7 squares: 136112 ranges, 30645 proofs; 901 queries on a
    batch of three squares: 10955 proofs
 f  25996 inclusion proofs and 76831 namespace proofs, valid and tampered, each
    through the host-pointer and the device-pointer batch
 g  one repair from a k x k sub-grid, one byzantine report

None of these found a fault in the kernels.  That the tests can fail was tried on
scratch builds, one edit each: two key words swapped in ns_key_load fail every
test of e and every namespace-verifier test of f; ns[3] left out of
ns_is_parity's AND fails tests of a, b, c, d, e and f, each on an edges square;
the byte-28 mask of the leaf kernel's namespace words dropped fails
test_node_stores_hold_every_subtree_root alone (the records' padding), since
ns_less and ns_is_parity mask again and the hashes never read bytes 29..31; with
ns_less's mask dropped as well the runs squares are flagged as out of order and
the tests of a, b, c, e and f that hold one fail.  (load_ns of nmt.hip has no caller.)"""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))
import oracle  # noqa: E402
import pyref  # noqa: E402
import nmt_namespace_model as model  # noqa: E402
import ns_corpus as corpus  # noqa: E402
from celestia_da import _abi, da, device, inclusion, proof, trees  # noqa: E402

pytestmark = pytest.mark.gpu

OK, ERR_PROOF, ERR_PUSH_ORDER = _abi.OK, _abi.ERR_PROOF, _abi.ERR_PUSH_ORDER
PUSH_ORDER_BIT = 1


@pytest.fixture(scope="module")
def ctx():
    c = da.Context(0)
    yield c
    c.close()


# ---- the members and their references, built once ----------------------------------------

_MEMBERS = {
    "ladder": lambda k, layout, v: corpus.ladder(k, 1 + v, layout),
    "runs": lambda k, layout, v: corpus.runs(k, 11 + v, layout),
    "edges": lambda k, layout, v: corpus.edges(k, layout, v),
    "max_row_end": lambda k, layout, v: corpus.max_row_end(k, 4 + v),
}
_ods, _ref, _trees = {}, {}, {}


def member(name, k, layout="row", v=0):
    key = (name, k, layout, v)
    if key not in _ods:
        _ods[key] = _MEMBERS[name](k, layout, v)
        _ods[key].setflags(write=False)
    return key, _ods[key]


def reference(key):
    """(eds, row roots, column roots, dah) of a member from the oracle."""
    if key not in _ref:
        _ref[key] = oracle.extend_and_dah(_ods[key], key[1], nthreads=8)
    return _ref[key]


def ref_trees(key):
    """trees[axis][index] of a member, rebuilt with pyref; their roots are the oracle's."""
    if key not in _trees:
        eds, rr, cr, _ = reference(key)
        t = corpus.axis_trees(eds, key[1], model)
        assert b"".join(x.root for x in t[0]) == rr.tobytes() and b"".join(x.root for x in t[1]) == cr.tobytes()
        _trees[key] = t
    return _trees[key]


def valid_members(k):
    """The valid members of width k, layouts alternating."""
    out = [member("ladder", k, "row"), member("ladder", k, "col", 1), member("runs", k, "row"),
           member("runs", k, "col", 1)]
    if k >= 8:
        out += [member("edges", k, "row", 0), member("edges", k, "col", 1), member("edges", k, "col", 0),
                member("edges", k, "row", 1)]
    if k >= 4:
        out.append(member("max_row_end", k))
    return out


def _dev(b):
    return torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda() if len(b) else \
        torch.empty(0, dtype=torch.uint8, device="cuda")


# ---- a: roots, DAH, status ---------------------------------------------------------------

def _extend(ctx, k, batch):
    sq = device.DeviceSquares(k, len(batch), ctx=ctx)
    sq.load_ods(np.stack([np.ascontiguousarray(o).reshape(-1) for o in batch]))
    sq.extend()
    torch.cuda.synchronize()
    return sq


def _assert_equals_oracle(sq, keys):
    status = sq.status.cpu().numpy()
    eds, rr, cr, dah = (t.cpu().numpy() for t in (sq.eds, sq.row_roots, sq.col_roots, sq.dah))
    for i, key in enumerate(keys):
        oeds, orr, ocr, odah = reference(key)
        assert status[i] == 0, key
        assert eds[i].tobytes() == oeds.tobytes(), key
        bad = np.flatnonzero((rr[i] != orr).any(axis=1))
        assert bad.size == 0, (key, "row roots", bad[:8])
        bad = np.flatnonzero((cr[i] != ocr).any(axis=1))
        assert bad.size == 0, (key, "column roots", bad[:8])
        assert dah[i].tobytes() == odah, key


@pytest.mark.parametrize("k", [1, 2, 4, 8, 16, 32])
def test_extend_batches_of_three(ctx, k):
    ms = valid_members(k)
    ms += ms[:-len(ms) % 3]
    compared = 0
    for at in range(0, len(ms), 3):
        keys = [key for key, _ in ms[at:at + 3]]
        assert {key[2] for key in keys} == {"row", "col"}       # the per-square Q0 table stride matters
        _assert_equals_oracle(_extend(ctx, k, [ods for _, ods in ms[at:at + 3]]), keys)
        compared += 3
    assert compared >= 6


def test_extend_workload_width(ctx):
    """k = 128: the whole parity row of the edges square makes waves of the
    level-1 kernel take the all-parity arm inside Q0, from data."""
    k = 128
    ms = [member("edges", k, "row"), member("ladder", k, "col")]
    ns = corpus.namespaces(ms[0][1], k)
    assert all(x == corpus.PARITY for x in ns[k - 1]) and ns[k - 2][k // 2 - 1] != corpus.PARITY
    _assert_equals_oracle(_extend(ctx, k, [ods for _, ods in ms]), [key for key, _ in ms])


@pytest.mark.parametrize("k", [4, 16])
def test_host_entry(ctx, k):
    for key, ods in valid_members(k):
        eds = da.extend_shares(ods, ctx)
        dah = da.new_data_availability_header(eds)
        oeds, orr, ocr, odah = reference(key)
        assert eds.data.tobytes() == oeds.tobytes(), key
        assert b"".join(dah.row_roots) == orr.tobytes(), key
        assert b"".join(dah.column_roots) == ocr.tobytes(), key
        assert dah.hash() == odah, key


# ---- b: push order -----------------------------------------------------------------------

def _violating(k):
    """(label, ods) of every violating square of width k."""
    out = []
    for layout in ("row", "col"):
        for ods, axis, cls, byte in corpus.violations(corpus.ladder(k, 6, layout), k):
            out.append(((layout, axis, cls, byte), ods))
    out.append(("parity_then_smaller", corpus.parity_then_smaller(k, 6)))
    return out


@pytest.mark.parametrize("k", [8, 32])
def test_push_order_bit_in_exactly_that_slot(ctx, k):
    others = [member("ladder", k, "col", 1)[1], member("runs", k, "row")[1]]
    sq = device.DeviceSquares(k, 3, ctx=ctx)
    runs = 0
    for label, ods in _violating(k):
        for slot in range(3):
            batch = list(others)
            batch.insert(slot, ods)
            want = [PUSH_ORDER_BIT if corpus.out_of_order(o, k) else 0 for o in batch]
            assert want == [int(i == slot) for i in range(3)]
            sq.load_ods(np.stack([np.ascontiguousarray(o).reshape(-1) for o in batch]))
            sq.extend()
            assert sq.status.cpu().numpy().tolist() == want, (label, slot)
            runs += 1
    assert runs == 3 * 73


@pytest.mark.parametrize("k", [8, 32])
def test_valid_squares_are_not_flagged(ctx, k):
    ms = [m for m in valid_members(k) if m[0][0] in ("runs", "edges", "max_row_end")]
    assert len(ms) == 7 and all(corpus.out_of_order(ods, k) == [] for _, ods in ms)
    sq = _extend(ctx, k, [ods for _, ods in ms])
    assert sq.status.cpu().numpy().tolist() == [0] * len(ms)


def _forest_status(ctx, k, forest, wrapper):
    """(rc, per-tree status, roots) of dagpu_wrapper_roots (raw shares, tree t at
    axis index t mod k) or dagpu_nmt_roots (namespaced pushes)."""
    counts, buf, leaf_len = trees._pack(forest)
    roots = np.zeros((len(forest), 90), np.uint8)
    status = np.full(len(forest), 77, np.int32)
    L = ctx._L
    if wrapper:
        axes = np.array([t % k for t in range(len(forest))], dtype=np.uint32)
        rc = L.dagpu_wrapper_roots(ctx.handle, k, len(forest), _abi.addr(axes), _abi.addr(counts), _abi.addr(buf),
                                   leaf_len, _abi.addr(roots), _abi.addr(status))
    else:
        rc = L.dagpu_nmt_roots(ctx.handle, len(forest), _abi.addr(counts), _abi.addr(buf), leaf_len, _abi.PREFIX_NONE,
                               None, 1, _abi.addr(roots), _abi.addr(status))
    return rc, status, roots


def _q0_forest(ods, k):
    """The Q0 part of the k row trees, then of the k column trees: raw shares."""
    cell = [ods[i].tobytes() for i in range(k * k)]
    return [cell[t * k:(t + 1) * k] for t in range(k)] + [cell[t::k] for t in range(k)]


@pytest.mark.parametrize("k", [8, 32])
def test_forest_check_order_flags_exactly_the_violating_tree(ctx, k):
    for label, ods in _violating(k):
        (axis, t, _), = corpus.out_of_order(ods, k)
        want = np.zeros(2 * k, np.int32)
        want[axis * k + t] = ERR_PUSH_ORDER
        forest = _q0_forest(ods, k)
        for wrapper in (True, False):
            pushes = forest if wrapper else [[s[:29] + s for s in tr] for tr in forest]
            rc, status, _ = _forest_status(ctx, k, pushes, wrapper)
            assert rc == ERR_PUSH_ORDER and (status == want).all(), (label, wrapper, np.flatnonzero(status != want))
    # the Python entries raise for the tree, and not for its valid neighbour
    label, ods = _violating(k)[7]
    (axis, t, _), = corpus.out_of_order(ods, k)
    forest = _q0_forest(ods, k)
    with pytest.raises(da.ErrInvalidPushOrder):
        trees.wrapper_roots(k, [t], [forest[axis * k + t]], ctx)
    with pytest.raises(da.ErrInvalidPushOrder):
        trees.nmt_roots([[s[:29] + s for s in forest[axis * k + t]]], True, ctx)
    other = forest[(1 - axis) * k + t]
    want_root = pyref.nmt_root_generic([s[:29] + s for s in other])
    assert trees.wrapper_roots(k, [t], [other], ctx) == [want_root]
    assert trees.nmt_roots([[s[:29] + s for s in other]], True, ctx) == [want_root]
    # valid squares: no tree flagged, every partial root as pyref has it
    for key, ods in [m for m in valid_members(k) if m[0][0] in ("runs", "edges", "max_row_end")][:3 if k > 8 else 7]:
        forest = _q0_forest(ods, k)
        want_roots = [pyref.nmt_root_generic([s[:29] + s for s in tr]) for tr in forest]
        for wrapper in (True, False):
            pushes = forest if wrapper else [[s[:29] + s for s in tr] for tr in forest]
            rc, status, roots = _forest_status(ctx, k, pushes, wrapper)
            assert rc == OK and not status.any(), (key, wrapper)
            assert [r.tobytes() for r in roots] == want_roots, (key, wrapper)


# ---- c: the forest on 512-B shares; the node stores ----------------------------------------

@pytest.mark.parametrize("k", [8, 16])
def test_wrapper_roots_of_every_axis(ctx, k):
    w = 2 * k
    for key, _ in [member("ladder", k, "row"), member("ladder", k, "col", 1), member("edges", k, "row", 0),
                   member("edges", k, "col", 1)]:
        eds, rr, cr, _ = reference(key)
        rows = [[eds[r, c].tobytes() for c in range(w)] for r in range(w)]
        cols = [[eds[r, c].tobytes() for r in range(w)] for c in range(w)]
        got = trees.wrapper_roots(k, list(range(w)) * 2, rows + cols, ctx)
        assert b"".join(got[:w]) == rr.tobytes(), key
        assert b"".join(got[w:]) == cr.tobytes(), key


def _rec_to_node(rec):
    return rec[0:29].tobytes() + rec[32:61].tobytes() + rec[64:96].tobytes()


def test_node_stores_hold_every_subtree_root(ctx):
    k, w = 8, 16
    checked = 0
    for key, _ in [member("ladder", k, "col", 1), member("edges", k, "row", 0), member("edges", k, "row", 1)]:
        eds = reference(key)[0]
        tr = ref_trees(key)
        store = inclusion.EDSAxisNodes(k, eds, ctx)
        torch.cuda.synchronize()
        rows = store.nodes.cpu().numpy().reshape(-1, 96)
        cols = store.col_inner.cpu().numpy().reshape(-1, 96)
        assert not rows[:, 29:32].any() and not rows[:, 61:64].any()
        assert not cols[:, 29:32].any() and not cols[:, 61:64].any()
        base = 0
        for lvl in range(0, w.bit_length()):
            per = w >> lvl
            for t in range(w):
                for p in range(per):
                    assert _rec_to_node(rows[base + t * per + p]) == tr[0][t].subroot(p << lvl, (p + 1) << lvl), \
                        (key, "row", lvl, t, p)
                    if lvl:
                        assert _rec_to_node(cols[base - w * w + t * per + p]) == \
                            tr[1][t].subroot(p << lvl, (p + 1) << lvl), (key, "col", lvl, t, p)
                    checked += 1 + (lvl > 0)
            base += w * per
        assert base == len(rows)
        # the gather of the cacher: every inner node of every row tree, by (row, depth, position)
        cacher = inclusion.EDSSubTreeRootCacher(k, eds, ctx)
        req = [(t, d, p) for t in range(w) for d in range(4) for p in range(1 << d)]
        got = cacher.nodes_at(*zip(*req))
        assert got == [tr[0][t].subroot(p * (w >> d), (p + 1) * (w >> d)) for t, d, p in req]
        checked += len(req)
    assert checked == 3 * (w * (2 * w - 1) + w * (w - 1) + w * 15)


# ---- d: range proofs -----------------------------------------------------------------------

class Resident:
    """One member extended on the device, with its node stores."""

    def __init__(self, ctx, key):
        k = key[1]
        self.key, self.k, self.w = key, k, 2 * k
        self.sq = _extend(ctx, k, [_ods[key]])
        _assert_equals_oracle(self.sq, [key])
        self.nodes = inclusion.EDSAxisNodes(k, self.sq.eds[0], ctx)
        self.roots = torch.cat([self.sq.row_roots[0].reshape(-1), self.sq.col_roots[0].reshape(-1)])
        self.eds = reference(key)[0]


_resident = {}


def resident(ctx, key):
    if key not in _resident:
        _resident[key] = Resident(ctx, key)
    return _resident[key]


def _prove(ctx, s, reqs):
    """(nodes per proof, namespace per proof, shares per proof, desc) of nmt_prove_batch_device."""
    nodes, ns, shares, desc = device.nmt_prove_batch_device(s.nodes, reqs, eds=s.nodes.eds, ctx=ctx)
    torch.cuda.synchronize()
    nodes, ns, shares = nodes.cpu().numpy().tobytes(), ns.cpu().numpy().tobytes(), shares.cpu().numpy().tobytes()
    out = []
    for i, d in enumerate(desc.tolist()):
        out.append(([nodes[90 * j:90 * (j + 1)] for j in range(d[5], d[5] + d[4])], ns[29 * i:29 * (i + 1)],
                    [shares[512 * j:512 * (j + 1)] for j in range(d[3], d[3] + d[2])]))
    return out, desc


def _cells(eds, axis, index, a, b):
    return [(eds[index, j] if axis == 0 else eds[j, index]).tobytes() for j in range(a, b)]


def _assert_range_proofs(ctx, key, reqs):
    s = resident(ctx, key)
    tr = ref_trees(key)
    got, desc = _prove(ctx, s, reqs)
    single = 0
    for (axis, index, a, b), (nodes, ns, shares) in zip(reqs, got):
        t = tr[axis][index]
        assert nodes == t.range_proof(a, b), (key, axis, index, a, b)
        assert ns == t.ns[a] and shares == _cells(s.eds, axis, index, a, b), (key, axis, index, a, b)
        # the proof folds to the oracle's root
        assert model.fold(t.leaves[a:b], a, b, nodes, t.root), (key, axis, index, a, b)
        if len(set(t.ns[a:b])) == 1:
            assert model.verify_inclusion(ns, shares, a, b, nodes, t.root), (key, axis, index, a, b)
            single += 1
    assert 0 < single < len(reqs)
    return got, desc


@pytest.mark.parametrize("name,layout,v", [("ladder", "col", 1), ("edges", "row", 0), ("edges", "row", 1)])
def test_every_range_proof_of_both_axes(ctx, name, layout, v):
    k, w = 8, 16
    key, _ = member(name, k, layout, v)
    reqs = [(axis, index, a, b) for index in range(w) for a in range(w) for b in range(a + 1, w + 1) for axis in (0, 1)]
    assert len(reqs) == 2 * w * (w * (w + 1) // 2)
    _assert_range_proofs(ctx, key, reqs)


def test_sampled_range_proofs_at_32(ctx):
    k, w = 32, 64
    rng = random.Random(32)
    for key, _ in [member("ladder", k, "col", 1), member("edges", k, "row", 0)]:
        reqs = []
        for axis in (0, 1):
            for index in range(w):
                for _ in range(6):
                    a = rng.randrange(w)
                    reqs.append((axis, index, a, rng.randrange(a + 1, w + 1)))
                reqs += [(axis, index, 0, w), (axis, index, k - 1, k + 1)]
        _assert_range_proofs(ctx, key, reqs)


# ---- e: namespace search and proofs ------------------------------------------------------

def _popcount(v):
    return bin(int(v)).count("1")


def _counts(want, m):
    hit = want[want[:, :, 0] != model.OUTSIDE]
    present = hit[hit[:, 0] == model.PRESENT]
    return [len(hit), int((hit[:, 0] == model.ABSENT).sum()),
            sum(_popcount(s) + m - _popcount(e - 1) for _, s, e in hit), int((present[:, 2] - present[:, 1]).sum())]


_searched = {}


def searched(ctx, key):
    """(queries, the model's ranges, the model's proofs in (query, row) order) of a member."""
    if key not in _searched:
        k = key[1]
        qs = corpus.queries(_ods[key], k)
        want = model.model_ranges(_ods[key], k, qs)
        rows = ref_trees(key)[0]
        proofs = [(q, r) + model.prove_namespace(rows[r], qs[q])
                  for q in range(len(qs)) for r in range(2 * k) if want[q, r, 0] != model.OUTSIDE]
        assert all(p[2:5] == tuple(want[p[0], p[1]]) for p in proofs)
        _searched[key] = (qs, want, proofs)
    return _searched[key]


SEARCH_MEMBERS = [("ladder", 8, "row", 0), ("runs", 8, "col", 1), ("edges", 8, "col", 1), ("edges", 8, "row", 0),
                  ("ladder", 16, "col", 1), ("runs", 16, "row", 0), ("edges", 16, "row", 0)]


@pytest.mark.parametrize("name,k,layout,v", SEARCH_MEMBERS)
def test_namespace_ranges_and_proofs(ctx, name, k, layout, v):
    key, ods = member(name, k, layout, v)
    s = resident(ctx, key)
    qs, want, proofs = searched(ctx, key)
    w, m = 2 * k, (2 * k).bit_length() - 1
    ranges, counts = device.nmt_namespace_ranges_device(s.nodes, qs, ctx=ctx)
    assert ranges.shape == want.shape and (ranges == want).all(), \
        [(qs[q].hex(), r) for q, r, _ in np.argwhere(ranges != want)[:4]]
    assert counts.tolist() == _counts(want, m)
    kind = want[:, :, 0]
    assert (kind == model.PRESENT).any() and (kind == model.ABSENT).any() and (kind == model.OUTSIDE).any()
    nodes, ns, shares, hashes, desc, pairs, counts = device.nmt_prove_namespace_batch_device(s.nodes, qs, ctx=ctx)
    torch.cuda.synchronize()
    nodes, ns, hashes = (t.cpu().numpy().tobytes() for t in (nodes, ns, hashes))
    shares = shares.cpu().numpy().reshape(-1, 512)
    assert ns == b"".join(qs) and counts.tolist() == _counts(want, m)
    assert len(desc) == len(pairs) == len(proofs)
    flat = s.eds.reshape(w * w, 512)
    node_off = leaf_off = n_abs = 0
    for i, (q, r, kind, a, b, want_nodes, want_lh) in enumerate(proofs):
        absent = kind == model.ABSENT
        assert pairs[i].tolist() == [q, r]
        assert desc[i].tolist() == [a, b, 0 if absent else b - a, leaf_off, len(want_nodes), node_off, q, r,
                                    n_abs if absent else -1], (qs[q].hex(), r)
        assert nodes[90 * node_off:90 * (node_off + len(want_nodes))] == b"".join(want_nodes), (qs[q].hex(), r)
        if absent:
            assert hashes[90 * n_abs:90 * (n_abs + 1)] == want_lh, (qs[q].hex(), r)
            n_abs += 1
        else:
            assert (shares[leaf_off:leaf_off + b - a] == flat[r * w + a:r * w + b]).all(), (qs[q].hex(), r)
            leaf_off += b - a
        node_off += len(want_nodes)
    assert (len(nodes), len(shares), len(hashes)) == (90 * node_off, leaf_off, 90 * n_abs)


def test_namespace_proofs_across_three_squares(ctx):
    k, w = 8, 16
    keys = [member("ladder", k, "row")[0], member("runs", k, "col", 1)[0], member("edges", k, "col", 1)[0]]
    sq = _extend(ctx, k, [_ods[key] for key in keys])
    _assert_equals_oracle(sq, keys)
    store = sq.proof_store()
    qs = []
    for key in keys:
        qs += [q for q in corpus.queries(_ods[key], k) if q not in qs]
    want = np.stack([model.model_ranges(_ods[key], k, qs) for key in keys], axis=1)     # (q, square, row, 3)
    rows = [ref_trees(key)[0] for key in keys]
    expected = [(q, i, r) + model.prove_namespace(rows[i][r], qs[q]) for q in range(len(qs)) for i in range(3)
                for r in range(w) if want[q, i, r, 0] != model.OUTSIDE]
    counts, per = device.nmt_namespace_squares_count_device(store, qs, ctx=ctx)
    r = device.nmt_prove_namespace_squares_device(store, qs, ctx=ctx)
    torch.cuda.synchronize()
    assert per.tolist() == (want[..., 0] != model.OUTSIDE).sum(axis=2).tolist()
    assert counts.tolist() == r.counts.tolist() and r.counts[0] == len(expected)
    # a namespace of one square is searched for in the others as well
    assert ((per > 0).sum(axis=1) == 1).any() and ((per > 0).sum(axis=1) == 3).any()
    nodes, shares, hashes, roots = (t.cpu().numpy().tobytes() for t in (r.nodes, r.shares, r.leaf_hashes, r.axis_roots))
    assert r.namespaces.cpu().numpy().tobytes() == b"".join(qs)
    for i, (q, sqi, row, kind, a, b, want_nodes, want_lh) in enumerate(expected):
        d = r.desc[i].tolist()
        assert r.hits[i].tolist() == [q, sqi, row, kind, a, b], i
        assert d[:3] == [a, b, b - a if kind == model.PRESENT else 0] and d[4] == len(want_nodes) and d[6:8] == [q, i]
        assert nodes[90 * d[5]:90 * (d[5] + d[4])] == b"".join(want_nodes), (qs[q].hex(), sqi, row)
        assert roots[90 * i:90 * (i + 1)] == rows[sqi][row].root
        if kind == model.ABSENT:
            assert hashes[90 * d[8]:90 * d[8] + 90] == want_lh, (qs[q].hex(), sqi, row)
        else:
            assert d[8] == -1 and shares[512 * d[3]:512 * (d[3] + d[2])] == \
                b"".join(_cells(reference(keys[sqi])[0], 0, row, a, b)), (qs[q].hex(), sqi, row)


# ---- f: the verifiers ----------------------------------------------------------------------

def host_inclusion(nid, leaves, start, end, nodes, root):
    return OK if proof.NMTProof(start, end, list(nodes)).verify_inclusion(nid, leaves, root) else ERR_PROOF


def host_namespace(nid, leaves, start, end, nodes, leaf_hash, root):
    p = proof.NMTProof(start, end, list(nodes), leaf_hash)
    return OK if p.verify_namespace(nid, [nid + x for x in leaves], root) else ERR_PROOF


def _every_alignment(pk):
    """The packed 29-B namespace table is read at every byte alignment."""
    return pk.n_ns >= 4 and set((pk.desc[:, 6] % 4).tolist()) == {0, 1, 2, 3}


@pytest.mark.parametrize("name,layout,v", [("ladder", "col", 1), ("edges", "row", 0), ("edges", "row", 1)])
def test_inclusion_verifiers_on_range_proofs(ctx, name, layout, v):
    """The produced range proofs of every tree of both axes, every range, and the
    namespace tampers of every seventh single-namespace one."""
    k, w = 8, 16
    key, ods = member(name, k, layout, v)
    s = resident(ctx, key)
    tr = ref_trees(key)
    reqs = [(axis, index, a, b) for axis in (0, 1) for index in range(w) for a in range(w) for b in range(a + 1, w + 1)]
    got, _ = _prove(ctx, s, reqs)
    items, classes = [], []
    for n, ((axis, index, a, b), (nodes, ns, shares)) in enumerate(zip(reqs, got)):
        root = tr[axis][index].root
        items.append((ns, shares, a, b, nodes, root))
        one = len(set(tr[axis][index].ns[a:b])) == 1
        classes.append("valid" if one else "several_namespaces")
        if one and n % 7 == 0:
            for cls, bad_ns, bad_nodes in corpus.namespace_tampers(ns, nodes, n):
                items.append((bad_ns, shares, a, b, bad_nodes, root))
                classes.append(cls)
    want = np.array([OK if model.verify_inclusion(*it) else ERR_PROOF for it in items], np.int32)
    assert all((st == OK) == (c == "valid") for st, c in zip(want, classes))
    assert {c[:8] for c in classes} >= {"valid", "several_", "node_min", "node_max", "claimed_"}
    host = np.array([host_inclusion(*it) for it in items], np.int32)
    assert (host == want).all(), [classes[i] for i in np.flatnonzero(host != want)[:8]]
    pk = proof.pack_nmt_proofs([(proof.NMTProof(a, b, list(nodes)), ns, lv, root)
                                for ns, lv, a, b, nodes, root in items], 512)
    assert _every_alignment(pk)
    st = proof._run_nmt(pk, ctx)
    assert (st == want).all(), [classes[i] for i in np.flatnonzero(st != want)[:8]]
    st = device.nmt_verify_batch_device(pk.desc, _dev(pk.namespaces), _dev(pk.leaves), 512, _dev(pk.nodes),
                                        _dev(pk.roots), ctx=ctx).cpu().numpy()
    assert (st == want).all(), [classes[i] for i in np.flatnonzero(st != want)[:8]]


@pytest.mark.parametrize("name,k,layout,v", SEARCH_MEMBERS)
def test_namespace_verifiers_on_namespace_proofs(ctx, name, k, layout, v):
    """The produced namespace proofs, the tampers of the model and the namespace
    tampers of every third proof: both batch forms against the host verifier and
    the model."""
    key, ods = member(name, k, layout, v)
    s = resident(ctx, key)
    qs, _, proofs = searched(ctx, key)
    tr = ref_trees(key)[0]
    w = 2 * k
    # the proofs as the device produced them (test_namespace_ranges_and_proofs compares them with the model's)
    got = proof.prove_namespaces(s.nodes, qs)
    produced = {(q, row): (p, sh) for q, per_q in enumerate(got) for row, p, sh in per_q}
    assert len(produced) == len(proofs)
    items, classes = [], []
    step = 1 if k == 8 else 25
    cells_of = [_cells(s.eds, 0, r, 0, w) for r in range(w)]
    for n, (q, r, kind, a, b, want_nodes, want_lh) in enumerate(proofs):
        p, sh = produced[q, r]
        assert (p.start, p.end, p.nodes, p.leaf_hash) == (a, b, want_nodes, want_lh)
        t, cells = tr[r], cells_of[r]
        assert sh == (cells[a:b] if kind == model.PRESENT else [])
        items.append((qs[q], sh, a, b, p.nodes, p.leaf_hash, t.root))
        classes.append("valid")
        if n % step:
            continue
        for cls, (tl, ts, te, tn, th, troot) in model.tampers(t, cells, qs[q], kind, a, b, p.nodes, p.leaf_hash):
            items.append((qs[q], tl, ts, te, tn, th, troot))
            classes.append(cls)
        if n % (3 * step) == 0:
            for cls, bad_nid, bad_nodes in corpus.namespace_tampers(qs[q], p.nodes, n):
                items.append((bad_nid, sh, a, b, bad_nodes, p.leaf_hash, t.root))
                classes.append(cls + ("_absent" if kind == model.ABSENT else ""))
    # the empty proof of some rows a namespace is outside of
    for q in range(0, len(qs), 7):
        for r in (0, k, w - 1):
            if model.prove_namespace(tr[r], qs[q])[0] == model.OUTSIDE:
                items.append((qs[q], [], 0, 0, [], b"", tr[r].root))
                classes.append("valid")
    want = np.array([OK if model.verify_namespace(*it) else ERR_PROOF for it in items], np.int32)
    for st, c in zip(want, classes):
        # only an absence proof may survive a changed claim
        assert (st == OK) == (c == "valid") or (c.startswith("claimed") and c.endswith("_absent")), c
    assert {c[:8] for c in classes} >= {"node_min", "node_max", "claimed_"}
    host = np.array([host_namespace(*it) for it in items], np.int32)
    assert (host == want).all(), [classes[i] for i in np.flatnonzero(host != want)[:8]]
    pk = proof.pack_namespace_proofs([(proof.NMTProof(a, b, list(nodes), lh), nid, lv, root)
                                      for nid, lv, a, b, nodes, lh, root in items], 512)
    assert _every_alignment(pk) and pk.n_leaf_hashes > 0
    st = proof._run_namespace(pk, ctx)
    assert (st == want).all(), [classes[i] for i in np.flatnonzero(st != want)[:8]]
    st = device.nmt_verify_namespace_batch_device(pk.desc, _dev(pk.namespaces), _dev(pk.leaves), 512, _dev(pk.nodes),
                                                  _dev(pk.leaf_hashes), _dev(pk.roots), ctx=ctx).cpu().numpy()
    assert (st == want).all(), [classes[i] for i in np.flatnonzero(st != want)[:8]]


# ---- g: repair -----------------------------------------------------------------------------

def test_repair_from_a_sub_grid_and_a_flipped_namespace_byte(ctx):
    k, w = 8, 16
    key, _ = member("ladder", k, "col", 1)
    eds, rr, cr, _ = reference(key)
    rng = np.random.default_rng(8)
    rows, cols = np.sort(rng.choice(w, k, replace=False)), np.sort(rng.choice(w, k, replace=False))
    assert (rows < k).any() and (cols < k).any() and (rows >= k).any() and (cols >= k).any()
    present = np.zeros((w, w), bool)
    present[np.ix_(rows, cols)] = True
    have = eds * present[:, :, None]
    fixed, p = da.repair(have, present, rr, cr, ctx)
    assert p.all() and fixed.tobytes() == eds.tobytes()
    orc, ofixed, _, _ = oracle.repair_ex(have, present, k, rr, cr)
    assert orc == 0 and ofixed.tobytes() == eds.tobytes()
    # the roots of the repaired square, rebuilt
    dah = da.new_data_availability_header(da.extend_shares(fixed[:k, :k].reshape(k * k, 512), ctx))
    assert b"".join(dah.row_roots) == rr.tobytes() and b"".join(dah.column_roots) == cr.tobytes()
    # one surviving Q0 share with byte 3 of its namespace flipped
    r, c = int(rows[rows < k][0]), int(cols[cols < k][0])
    bad = have.copy()
    bad[r, c, 3] ^= 0x40
    orc, _, opres, obyz = oracle.repair_ex(bad, present, k, rr, cr)
    assert orc == _abi.ERR_BYZANTINE
    with pytest.raises(da.ErrByzantineData) as e:
        da.repair(bad, present, rr, cr, ctx)
    assert e.value.byz == obyz and (e.value.present == opres.astype(bool)).all()
