"""Packing of proofs into the flat arrays of dagpu_nmt_verify_batch /
dagpu_merkle_verify_batch (celestia_da.proof.pack_*), and the shape checks of
validate_batch, which never reach the library.  No GPU."""
import numpy as np
import pytest

from celestia_da import _abi, da, proof


def _node(tag):
    return bytes([tag]) * 90


def test_pack_nmt_descriptors_offsets_and_shared_tables():
    ns_a, ns_b = b"\x00" * 28 + b"\x01", b"\x00" * 28 + b"\x02"
    root_a, root_b = _node(0xA0), _node(0xB0)
    sh = [bytes([i]) * 512 for i in range(8)]
    items = [
        (proof.NMTProof(2, 4, [_node(1), _node(2)]), ns_a, sh[0:2], root_a),
        (proof.NMTProof(0, 4, []), ns_b, sh[2:6], root_b),          # a whole tree: no nodes
        (proof.NMTProof(3, 4, [_node(3), _node(4), _node(5)]), ns_a, sh[6:7], root_a),  # shares ns and root
        (proof.NMTProof(-1, 1, [_node(6)]), ns_b, sh[7:8], root_a),
    ]
    pk = proof.pack_nmt_proofs(items, 512)
    assert pk.desc.dtype == np.int64 and pk.desc.shape == (4, 8)
    assert pk.desc.tolist() == [
        [2, 4, 2, 0, 2, 0, 0, 0],
        [0, 4, 4, 2, 0, 2, 1, 1],
        [3, 4, 1, 6, 3, 2, 0, 0],
        [-1, 1, 1, 7, 1, 5, 1, 0],
    ]
    assert (pk.n_ns, pk.n_leaves, pk.n_nodes, pk.n_roots, pk.leaf_len) == (2, 8, 6, 2, 512)
    assert pk.namespaces == ns_a + ns_b and pk.roots == root_a + root_b
    assert pk.leaves == b"".join(sh)
    assert pk.nodes == b"".join(_node(i) for i in range(1, 7))
    # every descriptor lies inside the totals it is checked against
    for s, e, nl, lo, nn, no, ni, ri in pk.desc.tolist():
        assert 0 <= lo and lo + nl <= pk.n_leaves and 0 <= no and no + nn <= pk.n_nodes
        assert 0 <= ni < pk.n_ns and 0 <= ri < pk.n_roots


def test_pack_merkle_descriptors():
    root = b"\x11" * 32
    other = b"\x22" * 32
    items = [
        (proof.MerkleProof(4, 1, b"\x01" * 32, [b"\x0a" * 32, b"\x0b" * 32]), root, b"r" * 90),
        (proof.MerkleProof(1, 0, b"\x02" * 32, []), other, b"s" * 90),
        (proof.MerkleProof(4, 3, b"\x03" * 32, [b"\x0c" * 32, b"\x0d" * 32]), root, b"t" * 90),
    ]
    pk = proof.pack_merkle_proofs(items, 90)
    assert pk.desc.tolist() == [[1, 4, 2, 0, 0, 0], [0, 1, 0, 2, 1, 1], [3, 4, 2, 2, 2, 0]]
    assert (pk.n_leaves, pk.leaf_len, pk.n_aunts, pk.n_roots) == (3, 90, 4, 2)
    assert pk.roots == root + other
    assert pk.leaves == b"r" * 90 + b"s" * 90 + b"t" * 90
    assert pk.leaf_hashes == b"\x01" * 32 + b"\x02" * 32 + b"\x03" * 32
    assert pk.aunts == b"\x0a" * 32 + b"\x0b" * 32 + b"\x0c" * 32 + b"\x0d" * 32


def _share_proof(rows=3, per_row=2):
    """A multi-row ShareProof of the right shape (its hashes are never looked at)."""
    sps = [proof.NMTProof(1, 1 + per_row, [_node(r)]) for r in range(rows)]
    mps = [proof.MerkleProof(16, r, bytes(32), [bytes(32)] * 4) for r in range(rows)]
    rp = proof.RowProof([_node(0x40 + r) for r in range(rows)], mps, 0, rows - 1)
    return proof.ShareProof([bytes(512)] * (rows * per_row), sps, bytes(28), rp, 0)


def test_multi_row_share_proof_packs_one_descriptor_per_row():
    sp = _share_proof()
    ns = bytes([sp.namespace_version]) + sp.namespace_id
    items, cursor = [], 0
    for j, p in enumerate(sp.share_proofs):
        items.append((p, ns, sp.data[cursor:cursor + p.end - p.start], sp.row_proof.row_roots[j]))
        cursor += p.end - p.start
    pk = proof.pack_nmt_proofs(items, 512)
    assert pk.desc.tolist() == [[1, 3, 2, 0, 1, 0, 0, 0], [1, 3, 2, 2, 1, 1, 0, 1], [1, 3, 2, 4, 1, 2, 0, 2]]
    assert (pk.n_ns, pk.n_leaves, pk.n_nodes, pk.n_roots) == (1, 6, 3, 3)


def test_validate_batch_shape_errors_in_reference_order_without_the_library(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("a shape error must not reach the library")

    monkeypatch.setattr(_abi, "lib", no_library)
    monkeypatch.setattr(proof, "default_context", no_library)
    good = _share_proof()
    # each case breaks one check; the later checks are broken too, so the
    # reported error shows which one fires first
    a = _share_proof()
    a.share_proofs = a.share_proofs[:-1]          # count mismatch ...
    a.data = a.data[1:]                           # ... and a share too few
    b = _share_proof()
    b.data = b.data[1:]                           # share count ...
    b.share_proofs[0] = proof.NMTProof(-2, 0, [])  # ... same span, negative start
    c = _share_proof()
    c.share_proofs[1] = proof.NMTProof(-1, 1, [])  # negative start before the empty range below
    c.share_proofs[2] = proof.NMTProof(3, 1, [])
    c.data = c.data[:2]
    d = _share_proof()
    d.share_proofs[0] = proof.NMTProof(2, 2, [])
    d.share_proofs[1] = proof.NMTProof(0, 4, [])
    d.row_proof.end_row = 7
    e = _share_proof()
    e.row_proof.end_row = 7                       # rows vs row roots ...
    e.row_proof.proofs = e.row_proof.proofs[:-1]   # ... before proofs vs row roots
    f = _share_proof()
    f.row_proof.proofs = f.row_proof.proofs[:-1]
    cases = [a, b, c, d, e, f]
    want = [
        "the number of share proofs 2 must equal the number of row roots 3",
        "the number of shares 5 must equal the number of shares in share proofs 6",
        "proof index cannot be negative: -1",
        "proof total must be positive: 0",
        "the number of rows is different than the number of row roots",
        "the number of proofs is different than the number of row roots",
    ]
    got = proof.validate_batch(cases, bytes(32))
    assert [str(g) for g in got] == want
    for sp, g in zip(cases, got):
        assert isinstance(g, da.DAError) and g.code == _abi.ERR_PROOF
        with pytest.raises(da.DAError) as ei:
            sp.validate(bytes(32))
        assert str(ei.value) == str(g)
    # one data root per proof is accepted, a wrong count is not
    assert len(proof.validate_batch(cases, [bytes(32)] * len(cases))) == len(cases)
    with pytest.raises(da.DAError):
        proof.validate_batch(cases, [bytes(32)])
    assert proof.validate_batch([], bytes(32)) == []
    assert good.row_proof.end_row == 2
