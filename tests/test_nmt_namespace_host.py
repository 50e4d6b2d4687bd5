"""dagpu_nmt_verify_namespace (the host verifier, the specification of the GPU
batch) against the Python model of the rules in include/dagpu.h
(tests/nmt_namespace_model.py): presence proofs with completeness, absence
proofs and empty proofs on trees of 1 .. 64 leaves, with and without a parity
half, every query of the test set, and every tamper class.  The two "dropped
share" proofs pass dagpu_nmt_verify_inclusion: that is the gap VerifyNamespace
closes.  Also the class counts of the k = 8 test square, and the Python mirror
(NMTProof.verify_namespace)."""
import itertools

import numpy as np
import pytest

import nmt_namespace_model as model
from celestia_da import _abi, proof

OK, ERR_PROOF = _abi.OK, _abi.ERR_PROOF
SIZES = [1, 2, 3, 5, 6, 7, 8, 12, 16, 64]
LEAF_LEN = 40

ALL = {"drop_first", "drop_last", "empty_for_present", "empty_for_absent", "absent_right", "absent_left",
       "absent_with_leaves", "present_with_leaf_hash", "flipped_byte", "wrong_root", "node_removed",
       "empty_with_leaves"}
# what a tree of one leaf (no range of two, nothing absent, no node) and of two
# leaves (an absent namespace only before the last leaf) can show
ALLOWED = {1: {"empty_for_present", "present_with_leaf_hash", "flipped_byte", "wrong_root", "empty_with_leaves"},
           2: ALL - {"absent_right"}}


def _buf(b):
    return np.frombuffer(b, np.uint8) if len(b) else np.zeros(1, np.uint8)


def host_namespace(nid, leaves, start, end, nodes, leaf_hash, root):
    ln = len(leaves[0]) if leaves else 0
    ns, lv, nd, rt, lh = _buf(nid), _buf(b"".join(leaves)), _buf(b"".join(nodes)), _buf(root), _buf(leaf_hash)
    return _abi.lib().dagpu_nmt_verify_namespace(_abi.addr(ns), _abi.addr(lv), len(leaves), ln, start, end,
                                                 _abi.addr(nd), len(nodes), _abi.addr(lh) if leaf_hash else None,
                                                 _abi.addr(rt))


def host_inclusion(nid, leaves, start, end, nodes, root):
    ln = len(leaves[0]) if leaves else 0
    ns, lv, nd, rt = _buf(nid), _buf(b"".join(leaves)), _buf(b"".join(nodes)), _buf(root)
    return _abi.lib().dagpu_nmt_verify_inclusion(_abi.addr(ns), _abi.addr(lv), len(leaves), ln, start, end,
                                                 _abi.addr(nd), len(nodes), _abi.addr(rt))


def _trees(n, seed):
    """(tree, leaf data, runs) for n leaves: two run patterns, each without and with a parity half."""
    rng = np.random.default_rng(seed)
    out = []
    for pattern, parity in itertools.product(([2, 1, 3], [1, 2, 1, 1]), (False, True)):
        real = n - n // 2 if parity and n > 1 else (0 if parity else n)
        ns, j = [], 0
        for r in itertools.cycle(pattern):
            if len(ns) >= real:
                break
            ns += [model.ns_id(16 + 2 * j)] * min(r, real - len(ns))
            j += 1
        ns += [model.PARITY] * (n - real)
        data = [rng.integers(0, 256, LEAF_LEN, dtype=np.uint8).tobytes() for _ in range(n)]
        out.append((model.Tree([model.pyref.leaf(a, d) for a, d in zip(ns, data)]), data, max(j, 1)))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_host_verifier_equals_model(n):
    seen, kinds = set(), set()
    for tree, data, n_runs in _trees(n, 9000 + n):
        for nid in model.queries(n_runs):
            kind, s, e, nodes, lh = model.prove_namespace(tree, nid)
            kinds.add(kind)
            lv = data[s:e] if kind == model.PRESENT else []
            assert model.verify_namespace(nid, lv, s, e, nodes, lh, tree.root), (n, nid.hex(), kind)
            assert host_namespace(nid, lv, s, e, nodes, lh, tree.root) == OK, (n, nid.hex(), kind)
            for name, (tl, ts, te, tn, th, tr) in model.tampers(tree, data, nid, kind, s, e, nodes, lh):
                assert not model.verify_namespace(nid, tl, ts, te, tn, th, tr), (n, nid.hex(), name)
                assert host_namespace(nid, tl, ts, te, tn, th, tr) == ERR_PROOF, (n, nid.hex(), name)
                seen.add(name)
                if name in ("drop_first", "drop_last"):
                    # a correct range proof of fewer shares: the inclusion verifier cannot tell
                    assert model.verify_inclusion(nid, tl, ts, te, tn, tr)
                    assert host_inclusion(nid, tl, ts, te, tn, tr) == OK, (n, nid.hex(), name)
    assert seen == ALLOWED.get(n, ALL), (n, sorted(ALLOWED.get(n, ALL) - seen), sorted(seen - ALLOWED.get(n, ALL)))
    assert {model.OUTSIDE, model.PRESENT} <= kinds and (n == 1 or model.ABSENT in kinds)


def test_degenerate_ranges_and_arguments():
    tree, data, _ = _trees(8, 1)[0]
    nid = tree.ns[0]
    kind, s, e, nodes, lh = model.prove_namespace(tree, nid)
    lv = data[s:e]
    L = _abi.lib()
    assert host_namespace(nid, lv, s, e, nodes, b"", tree.root) == OK
    for ts, te in ((-1, e), (e, s), (s, (1 << 62) + 1), (s, (1 << 63) - 1)):
        assert host_namespace(nid, lv, ts, te, nodes, b"", tree.root) == ERR_PROOF, (ts, te)
    # start == end with nodes is no empty proof: rule 2 rejects it
    assert host_namespace(nid, [], 3, 3, nodes, b"", tree.root) == ERR_PROOF
    assert host_namespace(nid, [], 0, 0, [], tree.leaves[0], tree.root) == ERR_PROOF
    # an absence proof of two leaves
    assert host_namespace(model.ns_id(15), [], 0, 2, tree.range_proof(0, 2), tree.leaves[0], tree.root) == ERR_PROOF
    buf = _buf(nid)
    assert L.dagpu_nmt_verify_namespace(None, None, 0, 0, 0, 0, None, 0, None, _abi.addr(buf)) == _abi.ERR_ARG
    assert L.dagpu_nmt_verify_namespace(_abi.addr(buf), None, 1, 4, 0, 1, None, 0, None, _abi.addr(buf)) == _abi.ERR_ARG


def test_k8_square_class_counts():
    """The counts of the k = 8 test square depend on the namespaces alone."""
    k = 8
    ods = model.namespaced_square(k, 8, model.K8_RUNS)
    qs = model.queries(len(model.K8_RUNS))
    assert len(qs) == 26
    r = model.model_ranges(ods, k, qs)
    kind = r[:, :, 0]
    assert ((kind == 0).sum(), (kind == 1).sum(), (kind == 2).sum()) == (388, 22, 6)
    present = r[kind == 1]
    assert ((present[:, 1] == 0) & (present[:, 2] == 2 * k)).sum() == 8
    assert ((present[:, 1] == 0) & (present[:, 2] == k)).sum() == 3
    assert (present[:, 1] == 0).sum() == 16 and (present[:, 2] == k).sum() == 8


def test_python_mirror():
    tree, data, n_runs = _trees(12, 5)[1]
    for nid in model.queries(n_runs):
        kind, s, e, nodes, lh = model.prove_namespace(tree, nid)
        p = proof.NMTProof(s, e, nodes, lh)
        assert p.is_empty_proof() == (kind == model.OUTSIDE) and p.is_of_absence() == (kind == model.ABSENT)
        lv = [nid + x for x in data[s:e]] if kind == model.PRESENT else []
        assert p.verify_namespace(nid, lv, tree.root)
        if kind == model.PRESENT:
            # nmt's own check: every leaf starts with the namespace
            assert not p.verify_namespace(nid, [tree.ns[(s + 1) % 2] + lv[0][29:]] + lv[1:], tree.root) or \
                tree.ns[(s + 1) % 2] == nid
            assert not p.verify_namespace(nid, [model.flip(lv[0], 3)] + lv[1:], tree.root)
            if e - s >= 2:
                q = proof.NMTProof(s + 1, e, tree.range_proof(s + 1, e))
                assert not q.verify_namespace(nid, lv[1:], tree.root)
                assert q.verify_inclusion(nid, [x[29:] for x in lv[1:]], tree.root)
        assert not p.verify_namespace(nid[:28], lv, tree.root)
