"""The full-width namespace corpus (tests/ns_corpus.py) on the host: the
properties the GPU tests rely on (conditions on the inputs: a seed that misses
one is replaced, not excused), the agreement of the two CPU references on every
member, and the library's host verifiers (dagpu_nmt_verify_inclusion,
dagpu_nmt_verify_namespace: the specification of the GPU batch verifiers)
against the Python model on trees of these squares."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))
import oracle  # noqa: E402
import pyref  # noqa: E402
import nmt_namespace_model as model  # noqa: E402
import ns_corpus as corpus  # noqa: E402
from celestia_da import _abi, proof  # noqa: E402

OK, ERR_PROOF = _abi.OK, _abi.ERR_PROOF
LADDER_SEEDS = (1, 2, 3)


# ---- corpus properties -------------------------------------------------------------------

def _first_differences(ods, k):
    """(row, column): the first differing bytes of adjacent Q0 pairs along each axis."""
    ns = corpus.namespaces(ods, k)
    row = {corpus.first_difference(ns[t][p], ns[t][p + 1]) for t in range(k) for p in range(k - 1)}
    col = {corpus.first_difference(ns[p][t], ns[p + 1][t]) for t in range(k) for p in range(k - 1)}
    return row, col


@pytest.mark.parametrize("k", [8, 16, 32])
def test_ladder_puts_a_first_difference_at_every_byte(k):
    row, col = set(), set()
    for seed in LADDER_SEEDS:
        for layout in ("row", "col"):
            ods = corpus.ladder(k, seed, layout)
            assert corpus.out_of_order(ods, k) == []
            r, c = _first_differences(ods, k)
            row |= r
            col |= c
    assert set(range(29)) <= row and set(range(29)) <= col
    # the stem itself occurs more than once: runs of equal namespaces
    assert None in row | col


def test_layouts_are_transposes_and_valid():
    for k in (1, 2, 4, 8):
        a, b = corpus.ladder(k, 5, "row"), corpus.ladder(k, 5, "col")
        assert (a.reshape(k, k, 512) == b.reshape(k, k, 512).transpose(1, 0, 2)).all()
        assert corpus.out_of_order(a, k) == corpus.out_of_order(b, k) == []
        assert k < 4 or not (a == b).all()


@pytest.mark.parametrize("k", [8, 16])
def test_runs_cross_row_ends_and_descend_behind_the_namespace(k):
    for layout in ("row", "col"):
        ods = corpus.runs(k, 11, layout)
        assert corpus.out_of_order(ods, k) == []
        grid = ods.reshape(k, k, 512)
        if layout == "col":
            grid = grid.transpose(1, 0, 2)
        flat = grid.reshape(k * k, 512)
        same = (flat[1:, :29] == flat[:-1, :29]).all(axis=1)
        assert same[np.arange(k - 1, k * k - 1, k)].any()          # a run crosses a row end
        lengths = np.diff(np.flatnonzero(np.concatenate([[True], ~same, [True]])))
        assert lengths.max() > k and lengths.min() == 1 and lengths.max() <= 2 * k
        # equal namespaces whose bytes 29..31 descend, next to each other on both axes
        def descends(x, y):
            return (x[..., :29] == y[..., :29]).all(axis=-1) & (x[..., 29] == 0xFF) & (y[..., 29] == 0x00)
        g = ods.reshape(k, k, 512)
        assert descends(g[:, :-1], g[:, 1:]).any() and descends(g[:-1], g[1:]).any()
        # and no namespace has zero bytes 0..18
        assert all(any(x[:19]) for row in corpus.namespaces(ods, k) for x in row)


@pytest.mark.parametrize("k", [8, 16, 128])
def test_edges_holds_the_near_namespaces_and_parity_rows(k):
    for layout in ("row", "col"):
        held = set()
        for part in (0, 1):
            ods = corpus.edges(k, layout, part)
            assert corpus.out_of_order(ods, k) == []
            ns = corpus.namespaces(ods, k)
            here = {x for row in ns for x in row}
            if k > 8:
                assert set(corpus.NEAR) <= here
            held |= here
            grid = [[ns[r][c] == corpus.PARITY for c in range(k)] for r in range(k)]
            if layout == "col":
                grid = [list(x) for x in zip(*grid)]
            assert all(grid[k - 1]) and grid[k - 2] == [False] * (k - k // 2) + [True] * (k // 2)
            assert not any(any(row) for row in grid[:k - 2])
            flat = [x for row in (ns if layout == "row" else zip(*ns)) for x in row]
            assert flat == sorted(flat)
            if k > 8 or part == 0:
                assert flat[:29] == sorted(corpus.NEAR[:29])
            if k > 8 or part == 1:
                assert flat[-(k + k // 2) - 29:-(k + k // 2)] == corpus.NEAR[29:]
                assert flat[-(k + k // 2) - 1] == corpus.TAIL_PADDING
        assert set(corpus.NEAR) <= held and len(corpus.NEAR) == 58


def test_max_row_end():
    k = 8
    ods = corpus.max_row_end(k, 4)
    assert corpus.out_of_order(ods, k) == []
    assert corpus.namespaces(ods, k)[k - 1][k - 1] == corpus.TAIL_PADDING


@pytest.mark.parametrize("layout", ["row", "col"])
@pytest.mark.parametrize("k", [8, 32])
def test_violations_have_one_out_of_order_pair(k, layout):
    base = corpus.ladder(k, 6, layout)
    seen = set()
    for ods, axis, cls, byte in corpus.violations(base, k):
        bad = corpus.out_of_order(ods, k)
        assert len(bad) == 1 and bad[0][0] == axis
        _, t, p = bad[0]
        assert cls == ("last_pair" if p == k - 2 else "even_odd" if p % 2 == 0 else "odd_even")
        ns = corpus.namespaces(ods, k)
        hi, lo = (ns[t][p], ns[t][p + 1]) if axis == 0 else (ns[p][t], ns[p + 1][t])
        assert lo < hi and corpus.first_difference(hi, lo) == byte
        if byte < 28:
            assert hi[byte + 1:] < lo[byte + 1:]       # the bytes behind order the other way
        assert (ods != base).any(axis=1).sum() == 1
        seen.add((axis, cls, byte))
    assert seen == {(a, c, b) for a in (0, 1) for c in corpus.POSITION_CLASSES for b in corpus.VIOLATION_BYTES}
    ods = corpus.parity_then_smaller(k, 6)
    assert corpus.out_of_order(ods, k) == [(0, k - 1, k // 2)]


def test_queries():
    k = 8
    ods = corpus.ladder(k, 1, "row")
    qs = corpus.queries(ods, k)
    own = {ods[i, :29].tobytes() for i in range(k * k)}
    assert len(set(qs)) == len(qs) and own <= set(qs) and set(corpus.NEAR) <= set(qs)
    flipped = {corpus.first_difference(q, x) for x in own for q in qs
               if q not in own and sum(a != b for a, b in zip(q, x)) == 1}
    assert all(any(p // 8 == word for p in flipped) for word in range(4))


# ---- the two references ------------------------------------------------------------------

def _valid_members(k):
    out = [("ladder", corpus.ladder(k, s, lay)) for s in LADDER_SEEDS[:2] for lay in ("row", "col")]
    out += [("runs", corpus.runs(k, 11, lay)) for lay in ("row", "col")]
    if k >= 8:
        out += [("edges", corpus.edges(k, lay, part)) for lay in ("row", "col") for part in (0, 1)]
    if k >= 4:
        out.append(("max_row_end", corpus.max_row_end(k, 4)))
    return out


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_oracle_equals_pyref_on_valid_members(k):
    for name, ods in _valid_members(k):
        eds, rr, cr, dah = oracle.extend_and_dah(ods, k)
        peds, prr, pcr, pdah = pyref.extend_and_dah([ods[i].tobytes() for i in range(k * k)], k)
        assert eds.tobytes() == b"".join(b"".join(row) for row in peds), name
        assert rr.tobytes() == b"".join(prr) and cr.tobytes() == b"".join(pcr) and dah == pdah, name


@pytest.mark.parametrize("k", [4, 8])
def test_oracle_rejects_exactly_the_violating_squares(k):
    n = 0
    for layout in ("row", "col"):
        for ods, axis, cls, byte in corpus.violations(corpus.ladder(k, 6, layout), k):
            with pytest.raises(oracle.OracleError):
                oracle.extend_and_dah(ods, k)
            n += 1
    assert n == 72
    with pytest.raises(oracle.OracleError):
        oracle.extend_and_dah(corpus.parity_then_smaller(k, 6), k)
    for name, ods in _valid_members(k):
        oracle.extend_and_dah(ods, k)


# ---- host verifiers against the model ----------------------------------------------------

def host_inclusion(nid, leaves, start, end, nodes, root):
    return OK if proof.NMTProof(start, end, list(nodes)).verify_inclusion(nid, leaves, root) else ERR_PROOF


def host_namespace(nid, leaves, start, end, nodes, leaf_hash, root):
    p = proof.NMTProof(start, end, list(nodes), leaf_hash)
    return OK if p.verify_namespace(nid, [nid + x for x in leaves], root) else ERR_PROOF


def _row_tree(ods, k, row):
    eds, rr, _, _ = oracle.extend_and_dah(ods, k)
    tree = corpus.axis_trees(eds, k, model)[0][row]
    assert tree.root == rr[row].tobytes()
    return tree, [eds[row, c].tobytes() for c in range(2 * k)]


@pytest.mark.parametrize("member", ["ladder", "edges0", "edges1"])
def test_host_verifiers_equal_model_on_every_range(member):
    k = 8
    # the ladder row with the run of equal namespaces; the edges rows that are half parity
    ods, row = {"ladder": (corpus.ladder(k, 1, "row"), None), "edges0": (corpus.edges(k, "row", 0), k - 2),
                "edges1": (corpus.edges(k, "row", 1), k - 2)}[member]
    if row is None:
        ns = corpus.namespaces(ods, k)
        row = next(r for r in range(k) if len(set(ns[r])) < k)
    tree, cells = _row_tree(ods, k, row)
    w = 2 * k
    verdicts = set()
    for s in range(w):
        for e in range(s + 1, w + 1):
            nodes = tree.range_proof(s, e)
            for nid in {tree.ns[s], tree.ns[e - 1]}:
                want = model.verify_inclusion(nid, cells[s:e], s, e, nodes, tree.root)
                assert want == (set(tree.ns[s:e]) == {nid})
                assert host_inclusion(nid, cells[s:e], s, e, nodes, tree.root) == (OK if want else ERR_PROOF), (s, e)
                want_ns = model.verify_namespace(nid, cells[s:e], s, e, nodes, b"", tree.root)
                # IgnoreMaxNamespace: a node that ends in parity leaves hides them from its max
                if nid != corpus.PARITY:
                    assert want_ns == (want and [i for i, x in enumerate(tree.ns) if x == nid] == list(range(s, e)))
                assert host_namespace(nid, cells[s:e], s, e, nodes, b"", tree.root) == (OK if want_ns else ERR_PROOF), \
                    (s, e)
                verdicts.add((want, want_ns))
                if want:
                    for name, bad_nid, bad_nodes in corpus.namespace_tampers(nid, nodes, s * w + e):
                        assert not model.verify_inclusion(bad_nid, cells[s:e], s, e, bad_nodes, tree.root), name
                        assert host_inclusion(bad_nid, cells[s:e], s, e, bad_nodes, tree.root) == ERR_PROOF, \
                            (s, e, name)
                        assert not model.verify_namespace(bad_nid, cells[s:e], s, e, bad_nodes, b"", tree.root), name
                        assert host_namespace(bad_nid, cells[s:e], s, e, bad_nodes, b"", tree.root) == ERR_PROOF, \
                            (s, e, name)
    assert verdicts == {(True, True), (True, False), (False, False)}


@pytest.mark.parametrize("member", ["ladder", "edges0", "edges1"])
def test_host_namespace_verifier_equals_model_on_every_query(member):
    k = 8
    ods = {"ladder": corpus.ladder(k, 1, "row"), "edges0": corpus.edges(k, "row", 0),
           "edges1": corpus.edges(k, "row", 1)}[member]
    qs = corpus.queries(ods, k)
    kinds = set()
    for row in (0, k - 2, k - 1, k):
        tree, cells = _row_tree(ods, k, row)
        for i, nid in enumerate(qs):
            kind, s, e, nodes, lh = model.prove_namespace(tree, nid)
            kinds.add(kind)
            lv = cells[s:e] if kind == model.PRESENT else []
            assert model.verify_namespace(nid, lv, s, e, nodes, lh, tree.root), (row, nid.hex())
            assert host_namespace(nid, lv, s, e, nodes, lh, tree.root) == OK, (row, nid.hex())
            for name, (tl, ts, te, tn, th, tr) in model.tampers(tree, cells, nid, kind, s, e, nodes, lh):
                assert not model.verify_namespace(nid, tl, ts, te, tn, th, tr), (row, nid.hex(), name)
                assert host_namespace(nid, tl, ts, te, tn, th, tr) == ERR_PROOF, (row, nid.hex(), name)
            if kind == model.OUTSIDE:
                continue
            for name, bad_nid, bad_nodes in corpus.namespace_tampers(nid, nodes, i):
                want = model.verify_namespace(bad_nid, lv, s, e, bad_nodes, lh, tree.root)
                # a changed node never verifies, nor do shares under a changed claim; an absence
                # proof may hold for the changed claim as well
                assert not want or (kind == model.ABSENT and name.startswith("claimed")), (row, nid.hex(), name)
                assert host_namespace(bad_nid, lv, s, e, bad_nodes, lh, tree.root) == (OK if want else ERR_PROOF), \
                    (row, nid.hex(), name)
    assert kinds == {model.OUTSIDE, model.PRESENT, model.ABSENT}
