"""Share inclusion proofs, host-side mirror of

  proof.NewShareInclusionProof      pkg/proof/proof.go:58-165
  proof.NewTxInclusionProof         pkg/proof/proof.go:23-54 (square built by celestia_da.square)
  proof.ParseNamespace              pkg/proof/querier.go:123-151
  merkle.ProofsFromByteSlices       celestia-core crypto/merkle (used at proof.go:87)
  nmt ProveRange                    nmt v0.20.0 (used at proof.go:139 via the wrapper tree)
  verification: ShareProof.Validate / VerifyProof, RowProof.Validate (celestia-core
  types/share_proof.go, row_proof.go), merkle Proof.Verify, nmt Proof.VerifyInclusion
  -> dagpu_merkle_verify / dagpu_nmt_verify_inclusion (host code of the library)
  many proofs at once (validate_batch, verify_inclusion_batch, merkle_verify_batch)
  -> dagpu_merkle_verify_batch / dagpu_nmt_verify_batch (hashed on the GPU)
  nmt ProveNamespace / Proof.VerifyNamespace, absence proofs included
  (celestia-node GetSharesByNamespace): NMTProof.verify_namespace,
  verify_namespace_batch, prove_namespaces, verify_namespace_data
  -> dagpu_nmt_verify_namespace(_batch), dagpu_nmt_prove_namespace_batch_device;
  the rules are stated in include/dagpu.h (recalled from nmt v0.20.0, parity unpinned)

The square is extended and hashed on the GPU, every row-tree node stays in HBM
(dagpu_row_nodes_device) and the RFC-6962 tree over rowRoots||colRoots is
built on the GPU with all levels (dagpu_merkle_levels); a proof is then a
selection of stored nodes (index arithmetic on the host, gathered on the
device).  No hashing happens on the host.

nmt's ProveRange emits the roots of the maximal subtrees that do not overlap
[start, end), left to right (its recursive buildRangeProof appends a subtree's
hash when the subtree is disjoint from the range and its parent is not);
merkle proofs list the sibling ("aunt") hashes from the leaf to the root.  The
node ORDER follows nmt v0.20.0 / celestia-core as restated here; the nmt module
is not in this image, so the proof byte layout is "parity unpinned" (the tests
re-derive every row root and the data root from the proofs).
"""
from __future__ import annotations

import ctypes
import hashlib
import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _abi
from .da import Context, DAError, default_context, extend_shares, new_data_availability_header
from .inclusion import EDSSubTreeRootCacher


# crypto/merkle MaxAunts (celestia-core v0.34 crypto/merkle/proof.go)
MAX_AUNTS = 100


@dataclass
class MerkleProof:
    """crypto/merkle Proof: Total, Index, LeafHash, Aunts (leaf to root)."""
    total: int
    index: int
    leaf_hash: bytes
    aunts: List[bytes]

    def verify(self, root: bytes, leaf: bytes) -> None:
        """merkle Proof.Verify: raises DAError when the proof does not prove
        `leaf` under `root`."""
        if root is None:
            raise DAError(_abi.ERR_ARG, "invalid root hash: cannot be nil")
        if self.total < 0:
            raise DAError(_abi.ERR_PROOF, "proof total must be positive")
        if self.index < 0:
            raise DAError(_abi.ERR_PROOF, "proof index cannot be negative")
        # Proof.ValidateBasic's MaxAunts bound, and Verify's LeafHash check
        if len(self.aunts) > MAX_AUNTS:
            raise DAError(_abi.ERR_PROOF, f"expected no more than {MAX_AUNTS} aunts, got {len(self.aunts)}")
        want_leaf = hashlib.sha256(b"\x00" + bytes(leaf)).digest()
        if bytes(self.leaf_hash) != want_leaf:
            raise DAError(_abi.ERR_PROOF, f"invalid leaf hash: wanted {want_leaf.hex().upper()} "
                                          f"got {bytes(self.leaf_hash).hex().upper()}")
        # keep every buffer referenced until the call returns (addr() is a raw pointer)
        r, lf, au = _bytes(root), _bytes(leaf), _bytes(b"".join(self.aunts))
        rc = _abi.lib().dagpu_merkle_verify(_abi.addr(r), _abi.addr(lf), len(leaf), self.index, self.total,
                                            _abi.addr(au), len(self.aunts))
        if rc == _abi.ERR_PROOF:
            raise DAError(rc, "invalid root hash")
        if rc:
            raise DAError(rc, "malformed merkle proof")


@dataclass
class NMTProof:
    """tmproto.NMTProof: Start, End (exclusive), Nodes (90-B), LeafHash (nil for inclusion)."""
    start: int
    end: int
    nodes: List[bytes]
    leaf_hash: bytes = b""

    def verify_inclusion(self, namespace: bytes, leaves: Sequence[bytes], root: bytes) -> bool:
        """nmt Proof.VerifyInclusion (IgnoreMaxNamespace): `leaves` are the raw
        shares (the tree prepends `namespace` to each)."""
        if len(namespace) != 29 or len(root) != 90 or any(len(n) != 90 for n in self.nodes):
            return False
        ln = len(leaves[0]) if leaves else 0
        if any(len(x) != ln for x in leaves):
            return False
        nsb, lv, nd, rt = _bytes(namespace), _bytes(b"".join(leaves)), _bytes(b"".join(self.nodes)), _bytes(root)
        rc = _abi.lib().dagpu_nmt_verify_inclusion(_abi.addr(nsb), _abi.addr(lv), len(leaves), ln, self.start,
                                                   self.end, _abi.addr(nd), len(self.nodes), _abi.addr(rt))
        return rc == 0

    def is_empty_proof(self) -> bool:
        """nmt Proof.IsEmptyProof: start == end, no nodes, no leaf hash."""
        return self.start == self.end and len(self.nodes) == 0 and len(self.leaf_hash) == 0

    def is_of_absence(self) -> bool:
        """nmt Proof.IsOfAbsence: the proof carries a leaf hash."""
        return len(self.leaf_hash) > 0

    def verify_namespace(self, nid: bytes, leaves: Sequence[bytes], root: bytes) -> bool:
        """nmt Proof.VerifyNamespace (IgnoreMaxNamespace): `leaves` are the
        tree's leaves WITH their 29-B namespace prefix (nid | share for a row
        tree); each must start with nid.  True iff the leaves are every leaf of
        nid under `root` (none for an absence or empty proof)."""
        raw = _strip_prefix(self, nid, leaves, root)
        if raw is None:
            return False
        ln = len(raw[0]) if raw else 0
        nsb, lv, nd, rt = _bytes(nid), _bytes(b"".join(raw)), _bytes(b"".join(self.nodes)), _bytes(root)
        lh = _bytes(self.leaf_hash)
        rc = _abi.lib().dagpu_nmt_verify_namespace(_abi.addr(nsb), _abi.addr(lv), len(raw), ln, _i64(self.start),
                                                   _i64(self.end), _abi.addr(nd), len(self.nodes),
                                                   _abi.addr(lh) if self.leaf_hash else None, _abi.addr(rt))
        return rc == 0


@dataclass
class RowProof:
    row_roots: List[bytes]
    proofs: List[MerkleProof]
    start_row: int
    end_row: int

    def validate(self, root: bytes) -> None:
        """RowProof.Validate: every row root is proven under the data root."""
        if self.end_row - self.start_row + 1 != len(self.row_roots):
            raise DAError(_abi.ERR_PROOF, "the number of rows is different than the number of row roots")
        if len(self.proofs) != len(self.row_roots):
            raise DAError(_abi.ERR_PROOF, "the number of proofs is different than the number of row roots")
        for p, r in zip(self.proofs, self.row_roots):
            try:
                p.verify(root, r)
            except DAError:
                raise DAError(_abi.ERR_PROOF, "row proof failed to verify") from None


@dataclass
class ShareProof:
    data: List[bytes]
    share_proofs: List[NMTProof]
    namespace_id: bytes
    row_proof: RowProof
    namespace_version: int

    def verify_proof(self) -> bool:
        """ShareProof.VerifyProof: each row's shares under its row root."""
        if self.namespace_version > 255:
            return False
        ns = bytes([self.namespace_version]) + self.namespace_id
        cursor = 0
        for i, p in enumerate(self.share_proofs):
            used = p.end - p.start
            if not p.verify_inclusion(ns, self.data[cursor:cursor + used], self.row_proof.row_roots[i]):
                return False
            cursor += used
        return True

    def validate(self, root: bytes) -> None:
        """ShareProof.Validate: shapes, the row proof under the data root, then
        the share proofs under the row roots."""
        n = sum(p.end - p.start for p in self.share_proofs)
        if len(self.share_proofs) != len(self.row_proof.row_roots):
            raise DAError(_abi.ERR_PROOF, f"the number of share proofs {len(self.share_proofs)} must equal the "
                                          f"number of row roots {len(self.row_proof.row_roots)}")
        if len(self.data) != n:
            raise DAError(_abi.ERR_PROOF, f"the number of shares {len(self.data)} must equal the number of "
                                          f"shares in share proofs {n}")
        for p in self.share_proofs:
            if p.start < 0:
                raise DAError(_abi.ERR_PROOF, f"proof index cannot be negative: {p.start}")
            if p.end - p.start <= 0:
                raise DAError(_abi.ERR_PROOF, f"proof total must be positive: {p.end - p.start}")
        self.row_proof.validate(root)
        if not self.verify_proof():
            raise DAError(_abi.ERR_PROOF, "share proof failed to verify")


def _bytes(b: bytes) -> np.ndarray:
    return np.frombuffer(b, np.uint8) if len(b) else np.zeros(1, np.uint8)


def _strip_prefix(p: "NMTProof", nid: bytes, leaves: Sequence[bytes], root: bytes) -> Optional[List[bytes]]:
    """The shape checks of verify_namespace and nmt's leaf[:29] == nID check;
    the leaves without their prefix, or None when a check fails."""
    if len(nid) != 29 or len(root) != 90 or any(len(n) != 90 for n in p.nodes) or len(p.leaf_hash) not in (0, 90):
        return None
    if any(len(x) < 29 or bytes(x[:29]) != bytes(nid) for x in leaves):
        return None
    raw = [bytes(x[29:]) for x in leaves]
    if any(len(x) != len(raw[0]) for x in raw):
        return None
    return raw


# ---------------------------------------------------------------------------
# Many proofs in one call (dagpu_nmt_verify_batch / dagpu_merkle_verify_batch):
# the hashing of ShareProof.Validate / RowProof.Validate for a whole list of
# proofs runs on the GPU; the reference consumer is VerifyShares
# (x/blobstream/client/verify.go:216-227).
# ---------------------------------------------------------------------------

@dataclass
class PackedNMT:
    """Flat arrays of dagpu_nmt_verify_batch for proofs of one leaf length.
    desc row = (start, end, n_leaves, leaf_off, n_nodes, node_off, ns_index,
    root_index); equal namespaces and equal roots are stored once."""
    desc: np.ndarray
    namespaces: bytes
    n_ns: int
    leaves: bytes
    n_leaves: int
    leaf_len: int
    nodes: bytes
    n_nodes: int
    roots: bytes
    n_roots: int


@dataclass
class PackedMerkle:
    """Flat arrays of dagpu_merkle_verify_batch for leaves of one length.
    desc row = (index, total, n_aunts, aunt_off, leaf_index, root_index)."""
    desc: np.ndarray
    leaves: bytes
    n_leaves: int
    leaf_len: int
    leaf_hashes: bytes
    aunts: bytes
    n_aunts: int
    roots: bytes
    n_roots: int


def _intern(table: dict, key: bytes) -> int:
    return table.setdefault(key, len(table))


def _i64(v: int) -> int:
    # a descriptor word is an int64: anything wider cannot be a valid proof
    # field and is clamped to a value the verifier rejects the same way
    return max(-(1 << 63), min((1 << 63) - 1, int(v)))


def pack_nmt_proofs(items: Sequence[Tuple[NMTProof, bytes, Sequence[bytes], bytes]], leaf_len: int) -> PackedNMT:
    """items: (proof, namespace, leaves, root) with 29-B namespaces, 90-B roots
    and nodes and leaves of leaf_len bytes (verify_inclusion_batch sorts out the
    others beforehand)."""
    nss, roots = {}, {}
    desc = np.zeros((len(items), 8), np.int64)
    leaves, nodes = [], []
    n_leaves = n_nodes = 0
    for i, (p, ns, lv, root) in enumerate(items):
        desc[i] = (_i64(p.start), _i64(p.end), len(lv), n_leaves, len(p.nodes), n_nodes,
                   _intern(nss, bytes(ns)), _intern(roots, bytes(root)))
        leaves.extend(bytes(x) for x in lv)
        nodes.extend(bytes(x) for x in p.nodes)
        n_leaves += len(lv)
        n_nodes += len(p.nodes)
    return PackedNMT(desc, b"".join(nss), len(nss), b"".join(leaves), n_leaves, leaf_len,
                     b"".join(nodes), n_nodes, b"".join(roots), len(roots))


def pack_merkle_proofs(items: Sequence[Tuple[MerkleProof, bytes, bytes]], leaf_len: int) -> PackedMerkle:
    """items: (proof, root, leaf) with 32-B roots, aunts and leaf hashes and
    leaves of leaf_len bytes."""
    roots = {}
    desc = np.zeros((len(items), 6), np.int64)
    aunts = []
    n_aunts = 0
    for i, (p, root, leaf) in enumerate(items):
        desc[i] = (_i64(p.index), _i64(p.total), len(p.aunts), n_aunts, i, _intern(roots, bytes(root)))
        aunts.extend(bytes(a) for a in p.aunts)
        n_aunts += len(p.aunts)
    return PackedMerkle(desc, b"".join(bytes(leaf) for _, _, leaf in items), len(items), leaf_len,
                        b"".join(bytes(p.leaf_hash) for p, _, _ in items), b"".join(aunts), n_aunts,
                        b"".join(roots), len(roots))


def _run_nmt(pk: PackedNMT, c: Context) -> np.ndarray:
    status = np.full(len(pk.desc), _abi.ERR_ARG, np.int32)
    desc = np.ascontiguousarray(pk.desc)
    ns, lv, nd, rt = _bytes(pk.namespaces), _bytes(pk.leaves), _bytes(pk.nodes), _bytes(pk.roots)
    c.check(c._L.dagpu_nmt_verify_batch(c.handle, len(desc), _abi.addr(desc), _abi.addr(ns), pk.n_ns,
                                        _abi.addr(lv), pk.n_leaves, pk.leaf_len, _abi.addr(nd), pk.n_nodes,
                                        _abi.addr(rt), pk.n_roots, _abi.addr(status)))
    return status


def _run_merkle(pk: PackedMerkle, c: Context) -> np.ndarray:
    status = np.full(len(pk.desc), _abi.ERR_ARG, np.int32)
    desc = np.ascontiguousarray(pk.desc)
    lv, lh, au, rt = _bytes(pk.leaves), _bytes(pk.leaf_hashes), _bytes(pk.aunts), _bytes(pk.roots)
    c.check(c._L.dagpu_merkle_verify_batch(c.handle, len(desc), _abi.addr(desc), _abi.addr(lv), pk.n_leaves,
                                           pk.leaf_len, _abi.addr(lh), _abi.addr(au), pk.n_aunts,
                                           _abi.addr(rt), pk.n_roots, _abi.addr(status)))
    return status


def _by_length(entries):
    """entries: (position, length, item) -> {length: [(position, item)]}."""
    groups = {}
    for pos, ln, it in entries:
        groups.setdefault(ln, []).append((pos, it))
    return groups


def verify_inclusion_batch(items: Sequence[Tuple[NMTProof, bytes, Sequence[bytes], bytes]],
                           ctx: Optional[Context] = None) -> List[bool]:
    """NMTProof.verify_inclusion for every (proof, namespace, leaves, root) of
    `items`, hashed on the GPU: one dagpu_nmt_verify_batch call per distinct
    leaf length (one call when all leaves are shares)."""
    out = [False] * len(items)
    entries = []
    for i, (p, ns, lv, root) in enumerate(items):
        if len(ns) != 29 or len(root) != 90 or any(len(n) != 90 for n in p.nodes):
            continue
        ln = len(lv[0]) if lv else 0
        if any(len(x) != ln for x in lv):
            continue
        entries.append((i, ln, (p, ns, lv, root)))
    if not entries:
        return out
    c = ctx or default_context()
    for ln, group in _by_length(entries).items():
        st = _run_nmt(pack_nmt_proofs([it for _, it in group], ln), c)
        for (pos, _), s in zip(group, st):
            out[pos] = int(s) == _abi.OK
    return out


@dataclass
class PackedNamespace(PackedNMT):
    """PackedNMT with 9-word descriptors (word 8 = leaf_hash_index, -1 = none)
    and the leaf-hash table of dagpu_nmt_verify_namespace_batch."""
    leaf_hashes: bytes = b""
    n_leaf_hashes: int = 0


def pack_namespace_proofs(items: Sequence[Tuple[NMTProof, bytes, Sequence[bytes], bytes]],
                          leaf_len: int) -> PackedNamespace:
    """items: (proof, nid, leaves WITHOUT prefix, root), shapes already checked."""
    nss, roots = {}, {}
    desc = np.zeros((len(items), _abi.NMT_NS_DESC_WORDS), np.int64)
    leaves, nodes, hashes = [], [], []
    n_leaves = n_nodes = 0
    for i, (p, ns, lv, root) in enumerate(items):
        lh = -1
        if p.leaf_hash:
            lh = len(hashes)
            hashes.append(bytes(p.leaf_hash))
        desc[i] = (_i64(p.start), _i64(p.end), len(lv), n_leaves, len(p.nodes), n_nodes,
                   _intern(nss, bytes(ns)), _intern(roots, bytes(root)), lh)
        leaves.extend(bytes(x) for x in lv)
        nodes.extend(bytes(x) for x in p.nodes)
        n_leaves += len(lv)
        n_nodes += len(p.nodes)
    return PackedNamespace(desc, b"".join(nss), len(nss), b"".join(leaves), n_leaves, leaf_len, b"".join(nodes),
                           n_nodes, b"".join(roots), len(roots), b"".join(hashes), len(hashes))


def _run_namespace(pk: PackedNamespace, c: Context) -> np.ndarray:
    status = np.full(len(pk.desc), _abi.ERR_ARG, np.int32)
    desc = np.ascontiguousarray(pk.desc)
    ns, lv, nd, rt, lh = (_bytes(pk.namespaces), _bytes(pk.leaves), _bytes(pk.nodes), _bytes(pk.roots),
                          _bytes(pk.leaf_hashes))
    c.check(c._L.dagpu_nmt_verify_namespace_batch(c.handle, len(desc), _abi.addr(desc), _abi.addr(ns), pk.n_ns,
                                                  _abi.addr(lv), pk.n_leaves, pk.leaf_len, _abi.addr(nd),
                                                  pk.n_nodes, _abi.addr(lh), pk.n_leaf_hashes, _abi.addr(rt),
                                                  pk.n_roots, _abi.addr(status)))
    return status


def _verify_namespace_raw(entries, out: List[bool], ctx: Optional[Context]) -> List[bool]:
    """entries: (position, leaf length, (proof, nid, leaves WITHOUT prefix, root))."""
    if not entries:
        return out
    c = ctx or default_context()
    for ln, group in _by_length(entries).items():
        st = _run_namespace(pack_namespace_proofs([it for _, it in group], ln), c)
        for (pos, _), s in zip(group, st):
            out[pos] = int(s) == _abi.OK
    return out


def verify_namespace_batch(items: Sequence[Tuple[NMTProof, bytes, Sequence[bytes], bytes]],
                           ctx: Optional[Context] = None) -> List[bool]:
    """NMTProof.verify_namespace for every (proof, nid, leaves with prefix,
    root) of `items`, hashed and folded on the GPU: one
    dagpu_nmt_verify_namespace_batch call per distinct leaf length (proofs
    without leaves go with length 0)."""
    out = [False] * len(items)
    entries = []
    for i, (p, nid, lv, root) in enumerate(items):
        raw = _strip_prefix(p, nid, lv, root)
        if raw is not None:
            entries.append((i, len(raw[0]) if raw else 0, (p, nid, raw, root)))
    return _verify_namespace_raw(entries, out, ctx)


def prove_namespaces(axis_nodes, namespaces: Sequence[bytes]) -> List[List[Tuple[int, NMTProof, List[bytes]]]]:
    """nmt ProveNamespace of every namespace on every row tree of one resident
    square (axis_nodes: inclusion.EDSAxisNodes): per namespace the list of
    (row, proof, shares) for the rows whose root range contains it -- presence
    proofs with their 512-B shares, absence proofs with none.  The other rows'
    proof is the empty proof and is not listed.  One
    dagpu_nmt_prove_namespace_batch_device call and one copy to the host."""
    from .device import nmt_prove_namespace_batch_device
    out: List[List[Tuple[int, NMTProof, List[bytes]]]] = [[] for _ in namespaces]
    if not len(namespaces):
        return out
    nodes, _, shares, hashes, desc, pairs, _ = nmt_prove_namespace_batch_device(axis_nodes, namespaces)
    nodes, shares, hashes = (t.cpu().numpy().tobytes() for t in (nodes, shares, hashes))
    for d, (q, row) in zip(desc, pairs):
        lh = hashes[90 * int(d[8]):90 * int(d[8]) + 90] if d[8] >= 0 else b""
        p = NMTProof(int(d[0]), int(d[1]), [nodes[90 * j:90 * (j + 1)] for j in range(int(d[5]), int(d[5] + d[4]))], lh)
        out[int(q)].append((int(row), p, [shares[512 * j:512 * (j + 1)] for j in range(int(d[3]), int(d[3] + d[2]))]))
    return out


def prove_namespaces_squares(store, namespaces: Sequence[bytes], stream=None):
    """prove_namespaces for every square of a device.ProofStore at once, and on
    to the data root: out[q][square] = list of (row, proof, shares, merkle) --
    the (row, proof, shares) of prove_namespaces(store.square(square), ...) and
    the MerkleProof of that row's root under the square's data root (leaf = the
    90-B row root, which proof.nodes fold to).  One
    dagpu_nmt_prove_namespace_squares_device call and one copy to the host."""
    import torch

    from .device import nmt_prove_namespace_squares_device
    out = [[[] for _ in range(store.n)] for _ in namespaces]
    if not len(namespaces):
        return out
    dev = store.store.device
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    r = nmt_prove_namespace_squares_device(store, namespaces, to_data_root=True, stream=s)
    parts = (r.nodes, r.shares, r.leaf_hashes, r.dah_leaf_hashes, r.aunts)
    with torch.cuda.stream(s):
        host = torch.cat(parts).cpu().numpy().tobytes()
    at = np.cumsum([0] + [t.numel() for t in parts])
    nodes, shares, hashes, dlh, aunts = (host[at[j]:at[j + 1]] for j in range(len(parts)))
    la = (2 * store.w).bit_length() - 1
    for i, (d, (q, sq, row, _, _, _)) in enumerate(zip(r.desc, r.hits)):
        lh = hashes[90 * int(d[8]):90 * int(d[8]) + 90] if d[8] >= 0 else b""
        p = NMTProof(int(d[0]), int(d[1]), [nodes[90 * j:90 * (j + 1)] for j in range(int(d[5]), int(d[5] + d[4]))], lh)
        mp = MerkleProof(2 * store.w, int(row), dlh[32 * i:32 * (i + 1)],
                         [aunts[32 * (i * la + a):32 * (i * la + a + 1)] for a in range(la)])
        out[int(q)][int(sq)].append(
            (int(row), p, [shares[512 * j:512 * (j + 1)] for j in range(int(d[3]), int(d[3] + d[2]))], mp))
    return out


def verify_namespace_data(row_roots: Sequence[bytes], nid: bytes,
                          rows: Sequence[Tuple[int, NMTProof, Sequence[bytes]]],
                          ctx: Optional[Context] = None) -> bool:
    """The light client's whole check of a GetSharesByNamespace answer: `rows`
    = (row, proof, shares) as prove_namespaces gives them (512-B shares, without
    the prefix the tree prepends).  True iff every row root whose [min, max]
    contains nid has exactly one entry and every entry verifies under its row
    root by VerifyNamespace, all in one batched call."""
    if len(nid) != 29 or any(len(r) != 90 for r in row_roots):
        return False
    seen = set()
    entries = []
    for i, (row, p, shares) in enumerate(rows):
        if not 0 <= row < len(row_roots) or row in seen:
            return False
        seen.add(row)
        if any(len(n) != 90 for n in p.nodes) or len(p.leaf_hash) not in (0, 90):
            return False
        ln = len(shares[0]) if shares else 0
        if any(len(x) != ln for x in shares):
            return False
        entries.append((i, ln, (p, nid, [bytes(x) for x in shares], bytes(row_roots[row]))))
    for row, root in enumerate(row_roots):
        if bytes(root[:29]) <= bytes(nid) <= bytes(root[29:58]) and row not in seen:
            return False
    return all(_verify_namespace_raw(entries, [False] * len(entries), ctx))


def merkle_verify_batch(items: Sequence[Tuple[MerkleProof, bytes, bytes]],
                        ctx: Optional[Context] = None) -> List[bool]:
    """MerkleProof.verify for every (proof, root, leaf): True where verify
    returns, False where it raises.  Leaf hashes, the LeafHash compare and the
    aunts run on the GPU: one dagpu_merkle_verify_batch call per distinct leaf
    length (one call for row roots)."""
    out = [False] * len(items)
    entries = []
    for i, (p, root, leaf) in enumerate(items):
        if root is None or len(root) != 32 or p.total < 0 or p.index < 0 or len(p.aunts) > MAX_AUNTS:
            continue
        if len(p.leaf_hash) != 32 or any(len(a) != 32 for a in p.aunts):
            continue
        entries.append((i, len(leaf), (p, root, leaf)))
    if not entries:
        return out
    c = ctx or default_context()
    for ln, group in _by_length(entries).items():
        st = _run_merkle(pack_merkle_proofs([it for _, it in group], ln), c)
        for (pos, _), s in zip(group, st):
            out[pos] = int(s) == _abi.OK
    return out


def _shape_error(p: "ShareProof") -> Optional[DAError]:
    """The checks ShareProof.validate and RowProof.validate make before any
    hash, in their order."""
    n = sum(sp.end - sp.start for sp in p.share_proofs)
    if len(p.share_proofs) != len(p.row_proof.row_roots):
        return DAError(_abi.ERR_PROOF, f"the number of share proofs {len(p.share_proofs)} must equal the "
                                       f"number of row roots {len(p.row_proof.row_roots)}")
    if len(p.data) != n:
        return DAError(_abi.ERR_PROOF, f"the number of shares {len(p.data)} must equal the number of "
                                       f"shares in share proofs {n}")
    for sp in p.share_proofs:
        if sp.start < 0:
            return DAError(_abi.ERR_PROOF, f"proof index cannot be negative: {sp.start}")
        if sp.end - sp.start <= 0:
            return DAError(_abi.ERR_PROOF, f"proof total must be positive: {sp.end - sp.start}")
    rp = p.row_proof
    if rp.end_row - rp.start_row + 1 != len(rp.row_roots):
        return DAError(_abi.ERR_PROOF, "the number of rows is different than the number of row roots")
    if len(rp.proofs) != len(rp.row_roots):
        return DAError(_abi.ERR_PROOF, "the number of proofs is different than the number of row roots")
    return None


def validate_batch(proofs: Sequence["ShareProof"], roots, ctx: Optional[Context] = None
                   ) -> List[Optional[DAError]]:
    """ShareProof.validate for every proof of a list: entry i is None where
    proofs[i].validate(root_i) returns and the DAError it raises otherwise.
    `roots` is one data root or one per proof.  The shape checks run here in the
    reference's order; every row proof of the list is then hashed by one
    merkle_verify_batch and every share proof by one verify_inclusion_batch."""
    if isinstance(roots, (bytes, bytearray)) or roots is None:
        roots = [roots] * len(proofs)
    if len(roots) != len(proofs):
        raise DAError(_abi.ERR_ARG, f"{len(roots)} data roots for {len(proofs)} proofs")
    out: List[Optional[DAError]] = [_shape_error(p) for p in proofs]
    m_items, m_owner, n_items, n_owner = [], [], [], []
    for i, (p, root) in enumerate(zip(proofs, roots)):
        if out[i] is not None:
            continue
        for mp, rr in zip(p.row_proof.proofs, p.row_proof.row_roots):
            m_items.append((mp, root, rr))
            m_owner.append(i)
        if p.namespace_version > 255:
            continue
        ns = bytes([p.namespace_version]) + p.namespace_id
        cursor = 0
        for j, sp in enumerate(p.share_proofs):
            used = sp.end - sp.start
            n_items.append((sp, ns, p.data[cursor:cursor + used], p.row_proof.row_roots[j]))
            n_owner.append(i)
            cursor += used
    row_bad, share_bad = set(), set()
    for i, ok in zip(m_owner, merkle_verify_batch(m_items, ctx) if m_items else []):
        if not ok:
            row_bad.add(i)
    for i, ok in zip(n_owner, verify_inclusion_batch(n_items, ctx) if n_items else []):
        if not ok:
            share_bad.add(i)
    for i, p in enumerate(proofs):
        if out[i] is not None:
            continue
        if i in row_bad:
            out[i] = DAError(_abi.ERR_PROOF, "row proof failed to verify")
        elif p.namespace_version > 255 or i in share_bad:
            out[i] = DAError(_abi.ERR_PROOF, "share proof failed to verify")
    return out


def merkle_levels(items: Sequence[bytes], ctx: Optional[Context] = None) -> List[List[bytes]]:
    """Every level of the RFC-6962 tree over `items` (level 0 = leaf hashes)."""
    c = ctx or default_context()
    n = len(items)
    if n == 0:
        return []
    ln = len(items[0])
    buf = np.frombuffer(b"".join(items), np.uint8) if ln else np.zeros(1, np.uint8)
    cap = ctypes.c_size_t(2 * n + 64)  # promoted odd nodes add <= log2(n)
    out = np.zeros((2 * n + 64, 32), np.uint8)
    c.check(c._L.dagpu_merkle_levels(c.handle, n, _abi.addr(buf), ln, _abi.addr(out), ctypes.byref(cap)))
    levels, off, cnt = [], 0, n
    while True:
        levels.append([out[off + i].tobytes() for i in range(cnt)])
        off += cnt
        if cnt == 1:
            return levels
        cnt = (cnt + 1) // 2


def proofs_from_byte_slices(items: Sequence[bytes], ctx: Optional[Context] = None
                            ) -> Tuple[bytes, List[MerkleProof]]:
    """merkle.ProofsFromByteSlices: (root, one proof per item)."""
    levels = merkle_levels(items, ctx)
    if not levels:
        raise DAError(_abi.ERR_ARG, "no items")
    proofs = []
    for i in range(len(items)):
        aunts, idx = [], i
        for lv in levels[:-1]:
            sib = idx ^ 1
            if sib < len(lv):  # an odd last node is promoted: no aunt at this level
                aunts.append(lv[sib])
            idx >>= 1
        proofs.append(MerkleProof(len(items), i, levels[0][i], aunts))
    return levels[-1][0], proofs


def range_proof_nodes(width: int, start: int, end: int) -> List[Tuple[int, int]]:
    """(depth, position) of the maximal subtrees of a full tree of `width`
    leaves disjoint from [start, end), left to right (nmt buildRangeProof)."""
    out: List[Tuple[int, int]] = []
    max_depth = int(math.log2(width))

    def rec(lo: int, hi: int, depth: int):
        if hi <= start or lo >= end:
            out.append((depth, lo >> (max_depth - depth)))
            return
        if hi - lo == 1:
            return
        mid = (lo + hi) // 2
        rec(lo, mid, depth + 1)
        rec(mid, hi, depth + 1)

    rec(0, width, 0)
    return out


def prove_row_ranges(cacher: EDSSubTreeRootCacher, ranges: Sequence[Tuple[int, int, int]]) -> List[NMTProof]:
    """ProveRange(start, end) on row trees: ranges = (row, start, end)."""
    reqs, spans = [], []
    for row, s, e in ranges:
        if not (0 <= s < e <= cacher.w):
            raise DAError(_abi.ERR_ARG, f"invalid range: [{s}, {e}) for a tree of {cacher.w} leaves")
        nodes = range_proof_nodes(cacher.w, s, e)
        spans.append((len(reqs), len(nodes)))
        reqs.extend((row, d, p) for d, p in nodes)
    got = cacher.nodes_at([r[0] for r in reqs], [r[1] for r in reqs], [r[2] for r in reqs])
    return [NMTProof(s, e, got[a:a + n]) for (row, s, e), (a, n) in zip(ranges, spans)]


def prove_ranges(axis_nodes, requests: Sequence[Tuple[int, int, int, int]]) -> List[NMTProof]:
    """ProveRange(start, end) on row (axis 0) and column (axis 1) trees of one
    resident square: requests = (axis, index, start, end), axis_nodes an
    inclusion.EDSAxisNodes.  One dagpu_nmt_prove_batch_device call and one copy
    to the host for the whole list; range_proof_nodes / prove_row_ranges stay
    the specification of the node order."""
    from .device import nmt_prove_batch_device
    if not len(requests):
        return []
    nodes, _, _, desc = nmt_prove_batch_device(axis_nodes, requests)
    host = nodes.cpu().numpy().tobytes()
    return [NMTProof(int(d[0]), int(d[1]), [host[90 * j:90 * (j + 1)] for j in range(int(d[5]), int(d[5] + d[4]))])
            for d in desc]


def new_share_inclusion_proof(shares: Sequence[bytes], namespace: bytes, share_range: Tuple[int, int],
                              ctx: Optional[Context] = None) -> ShareProof:
    """NewShareInclusionProof for a data square given as its k*k shares;
    share_range = [start, end) in row-major share order (pre-validated, as in
    the reference)."""
    c = ctx or default_context()
    n = len(shares)
    k = int(math.isqrt(n))
    start, end = share_range
    start_row, end_row = start // k, (end - 1) // k
    start_leaf, end_leaf = start % k, (end - 1) % k
    eds = extend_shares(np.frombuffer(b"".join(shares), np.uint8).reshape(n, 512), c)
    dah = new_data_availability_header(eds)
    _, all_proofs = proofs_from_byte_slices(dah.row_roots + dah.column_roots, c)
    cacher = EDSSubTreeRootCacher(k, eds.data, c)
    ranges, data = [], []
    for i, row in enumerate(range(start_row, end_row + 1)):
        s = start_leaf if i == 0 else 0
        e = end_leaf if row == end_row else k - 1
        ranges.append((row, s, e + 1))
        data.extend(eds.cell(row, j) for j in range(s, e + 1))
    return ShareProof(
        data=data,
        share_proofs=prove_row_ranges(cacher, ranges),
        namespace_id=namespace[1:],
        row_proof=RowProof(dah.row_roots[start_row:end_row + 1], all_proofs[start_row:end_row + 1],
                           start_row, end_row),
        namespace_version=namespace[0],
    )


def parse_namespace(raw_shares: Sequence[bytes], start_share: int, end_share: int) -> bytes:
    """proof.ParseNamespace (querier.go:123-151): the one namespace of shares
    [start_share, end_share)."""
    if start_share < 0:
        raise DAError(_abi.ERR_ARG, f"start share {start_share} should be positive")
    if end_share < 0:
        raise DAError(_abi.ERR_ARG, f"end share {end_share} should be positive")
    if end_share < start_share:
        raise DAError(_abi.ERR_ARG, f"end share {end_share} cannot be lower than starting share {start_share}")
    if end_share > len(raw_shares):
        raise DAError(_abi.ERR_ARG, f"end share {end_share} is higher than block shares {len(raw_shares)}")
    ns = bytes(raw_shares[start_share][:29])
    for i, share in enumerate(raw_shares[start_share:end_share]):
        if bytes(share[:29]) != ns:
            raise DAError(_abi.ERR_ARG, f"shares range contain different namespaces at index {i}: "
                                        f"{ns.hex()} and {bytes(share[:29]).hex()}")
    return ns


def new_tx_inclusion_proof(txs: Sequence[bytes], tx_index: int, app_version: int = 1,
                           ctx: Optional[Context] = None) -> ShareProof:
    """proof.NewTxInclusionProof: build the square from `txs`, find the tx's
    share range and prove it (the shares of a PFB live in the PFB namespace)."""
    from . import blobtx, shares as sh, square as sq
    if tx_index >= len(txs):
        raise DAError(_abi.ERR_ARG, f"txIndex {tx_index} out of bounds")
    b = sq.Builder(sq.square_size_upper_bound(app_version), app_version, *txs)
    data_square = b.export()
    r = b.find_tx_share_range(tx_index)
    _, is_blob = blobtx.unmarshal_blob_tx(txs[tx_index])
    ns = sh.PAY_FOR_BLOB_NAMESPACE if is_blob else sh.TX_NAMESPACE
    return new_share_inclusion_proof(data_square.square_bytes(), ns, (r.start, r.end), ctx)
