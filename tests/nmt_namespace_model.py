"""Python model of nmt ProveNamespace / Proof.VerifyNamespace as include/dagpu.h
states them (IgnoreMaxNamespace, 29-B namespaces), over the oracle's
pure-Python nmt hasher (pyref.leaf / pyref.node), and the test squares of
tests/test_nmt_namespace_host.py and tests/test_gpu_nmt_namespace.py.  A helper
module, not a test file."""
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))
import pyref  # noqa: E402
from celestia_da import synth  # noqa: E402

PARITY = b"\xff" * 29
OUTSIDE, PRESENT, ABSENT = 0, 1, 2


def ns_id(v: int) -> bytes:
    return b"\x00" * 19 + v.to_bytes(10, "big")


def split_point(n: int) -> int:
    k = 1
    while k * 2 < n:
        k *= 2
    return k


def hash_node(l: bytes, r: bytes):
    """nmt HashNode: None for unordered siblings."""
    if r[:29] < l[29:58]:
        return None
    return pyref.node(l, r)


class Tree:
    """One nmt over leaf nodes (90 B each) with nmt's split points."""

    def __init__(self, leaf_nodes):
        self.leaves = list(leaf_nodes)
        self.n = len(self.leaves)
        self.ns = [x[:29] for x in self.leaves]
        self._sub = {}
        self.root = self.subroot(0, self.n)

    def subroot(self, lo, hi):
        key = (lo, hi)
        if key not in self._sub:
            if hi - lo == 1:
                self._sub[key] = self.leaves[lo]
            else:
                mid = lo + split_point(hi - lo)
                self._sub[key] = pyref.node(self.subroot(lo, mid), self.subroot(mid, hi))
        return self._sub[key]

    def range_proof(self, start, end):
        """nmt buildRangeProof: roots of the maximal subtrees disjoint from [start, end)."""
        out = []

        def rec(lo, hi):
            if hi <= start or lo >= end:
                out.append(self.subroot(lo, hi))
                return
            if hi - lo == 1:
                return
            mid = lo + split_point(hi - lo)
            rec(lo, mid)
            rec(mid, hi)

        rec(0, self.n)
        return out


def find_range(ns, rmin, rmax, nid):
    """(kind, start, end) of ProveNamespace from the leaf namespaces and the root's range."""
    if nid < rmin or rmax < nid:
        return OUTSIDE, 0, 0
    hit = [i for i, x in enumerate(ns) if x == nid]
    if hit:
        assert hit == list(range(hit[0], hit[-1] + 1))
        return PRESENT, hit[0], hit[-1] + 1
    s = next(i for i, x in enumerate(ns) if x > nid)
    return ABSENT, s, s + 1


def prove_namespace(tree: Tree, nid: bytes):
    """(kind, start, end, nodes, leaf_hash)."""
    kind, s, e = find_range(tree.ns, tree.root[:29], tree.root[29:58], nid)
    if kind == OUTSIDE:
        return kind, 0, 0, [], b""
    return kind, s, e, tree.range_proof(s, e), tree.leaves[s] if kind == ABSENT else b""


def fold(lh, start, end, nodes, root, nid=None):
    """The fold of VerifyInclusion (nid None) / VerifyNamespace over leaf nodes lh."""
    state = {"leaf": 0, "node": 0, "ok": True}

    def complete(node, left):
        if nid is not None and not (node[29:58] < nid if left else nid < node[:29]):
            state["ok"] = False

    def root_of(lo, hi):
        if hi - lo == 1 and start <= lo < end:
            state["leaf"] += 1
            return lh[state["leaf"] - 1]
        if hi - lo == 1 or hi <= start or lo >= end:
            if state["node"] >= len(nodes):
                return None
            nd = nodes[state["node"]]
            state["node"] += 1
            complete(nd, hi <= start)
            return nd
        k = split_point(hi - lo)
        l = root_of(lo, lo + k)
        if l is None:
            return None
        r = root_of(lo + k, hi)
        if r is None:
            return l
        h = hash_node(l, r)
        if h is None:
            state["ok"] = False
            return pyref.node(l, r)
        return h

    est = 1
    while est < end:
        est *= 2
    acc = root_of(0, est)
    if acc is None:
        return False
    while state["node"] < len(nodes):
        nd = nodes[state["node"]]
        state["node"] += 1
        complete(nd, False)
        h = hash_node(acc, nd)
        if h is None:
            state["ok"] = False
            h = pyref.node(acc, nd)
        acc = h
    return state["ok"] and state["leaf"] == len(lh) and acc == root


def verify_namespace(nid, leaves, start, end, nodes, leaf_hash, root):
    """Proof.VerifyNamespace; `leaves` WITHOUT the namespace prefix."""
    if start == end and not nodes and not leaf_hash:
        return not leaves and (nid < root[:29] or root[29:58] < nid)
    if start < 0 or start >= end or end > 1 << 62:
        return False
    if leaf_hash:
        if leaves or end - start != 1 or not nid < leaf_hash[:29]:
            return False
        lh = [leaf_hash]
    else:
        if len(leaves) != end - start:
            return False
        lh = [pyref.leaf(nid, x) for x in leaves]
    return fold(lh, start, end, nodes, root, nid)


def verify_inclusion(nid, leaves, start, end, nodes, root):
    if start < 0 or start >= end or len(leaves) != end - start:
        return False
    return fold([pyref.leaf(nid, x) for x in leaves], start, end, nodes, root)


# ---- tampered proofs ---------------------------------------------------------------------

def flip(b, at):
    return b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]


def tampers(tree, data, nid, kind, s, e, nodes, lh):
    """(class, (leaves, start, end, nodes, leaf_hash, root)) for one valid proof."""
    root, n = tree.root, tree.n
    out = []
    if kind == PRESENT:
        lv = data[s:e]
        if e - s >= 2:
            out.append(("drop_first", (lv[1:], s + 1, e, tree.range_proof(s + 1, e), b"", root)))
            out.append(("drop_last", (lv[:-1], s, e - 1, tree.range_proof(s, e - 1), b"", root)))
        out.append(("empty_for_present", ([], 0, 0, [], b"", root)))
        out.append(("present_with_leaf_hash", (lv, s, e, nodes, tree.leaves[s], root)))
        out.append(("flipped_byte", ([flip(lv[0], 7)] + lv[1:], s, e, nodes, b"", root)))
        out.append(("empty_with_leaves", (lv, 0, 0, [], b"", root)))
    elif kind == ABSENT:
        lv = []
        out.append(("empty_for_absent", ([], 0, 0, [], b"", root)))
        if s + 1 < n:
            out.append(("absent_right", ([], s + 1, s + 2, tree.range_proof(s + 1, s + 2), tree.leaves[s + 1], root)))
        if s >= 1:
            out.append(("absent_left", ([], s - 1, s, tree.range_proof(s - 1, s), tree.leaves[s - 1], root)))
        out.append(("absent_with_leaves", ([data[s]], s, e, nodes, lh, root)))
    else:
        out.append(("empty_with_leaves", ([data[0]], 0, 0, [], b"", root)))
        return out
    out.append(("wrong_root", (lv, s, e, nodes, lh, flip(root, 70))))
    if nodes:
        out.append(("node_removed", (lv, s, e, nodes[:-1], lh, root)))
    return out


# ---- test squares ------------------------------------------------------------------------

K8_RUNS = [1, 7, 8, 3, 11, 2, 1, 1, 13, 9, 8]


def run_lengths(k: int, seed: int):
    """Seeded run lengths in 1 .. 2k that fill a k x k square (the last one cut)."""
    if k == 8:
        return list(K8_RUNS)
    rng, runs, left = random.Random(seed), [], k * k
    while left:
        r = min(rng.randint(1, 2 * k), left)
        runs.append(r)
        left -= r
    return runs


def namespaced_square(k: int, seed: int, runs):
    """synth.random_blob_square with bytes [0:29] of share i set to the namespace
    of its run: run j (row-major) has namespace 0x00*19 | be10(16 + 2j)."""
    assert sum(runs) == k * k
    ods = synth.random_blob_square(k, seed).copy()
    i = 0
    for j, r in enumerate(runs):
        ods[i:i + r, :29] = np.frombuffer(ns_id(16 + 2 * j), np.uint8)
        i += r
    return ods


def queries(n_runs: int):
    return ([b"\x00" * 29, ns_id(15)] + [ns_id(16 + 2 * j) for j in range(n_runs)]
            + [ns_id(17 + 2 * j) for j in range(n_runs)] + [b"\xff" * 28 + b"\xfe", PARITY])


def row_namespaces(ods, k: int):
    """Leaf namespaces of the 2k row trees of the extended square, from the ODS alone."""
    w = 2 * k
    rows = []
    for r in range(w):
        if r < k:
            rows.append([ods[r * k + c, :29].tobytes() for c in range(k)] + [PARITY] * k)
        else:
            rows.append([PARITY] * w)
    return rows


def root_range(ns):
    """(min, max) of the root of a tree with these leaf namespaces (IgnoreMaxNamespace)."""
    real = [x for x in ns if x != PARITY]
    return ns[0], (max(real) if real else PARITY)


def model_ranges(ods, k: int, qs):
    """(n_q, 2k, 3) int32: (kind, start, end) of every (query, row)."""
    rows = row_namespaces(ods, k)
    out = np.zeros((len(qs), 2 * k, 3), np.int32)
    for q, nid in enumerate(qs):
        for r, ns in enumerate(rows):
            out[q, r] = find_range(ns, *root_range(ns), nid)
    return out
