"""Share proofs to the data root from a whole batch of resident squares
(dagpu_proof_store_device, dagpu_nmt_prove_squares_device,
dagpu_share_proof_requests; device.ProofStore, device.nmt_prove_squares_device,
DeviceSquares.proof_store / share_proofs / blob_proofs).

The specification is the single-square route the batch replaces:
inclusion.EDSAxisNodes and device.nmt_prove_batch_device square by square,
hashlib for the RFC-6962 tree over rowRoots || colRoots,
proof.proofs_from_byte_slices for the aunts and proof.new_share_inclusion_proof
for whole ShareProofs.  Batches hold 3 squares from three seeds, so that a wrong
square index cannot pass."""
import ctypes
import hashlib
import random

import numpy as np
import pytest
import torch

from celestia_da import _abi, da, device, inclusion, proof, square as sq, synth
from celestia_da.da import DAError

pytestmark = pytest.mark.gpu

OK, ERR_PROOF, ERR_ARG = _abi.OK, _abi.ERR_PROOF, _abi.ERR_ARG


@pytest.fixture(scope="module")
def ctx():
    c = da.Context(0)
    yield c
    c.close()


def _one_namespace_square(k, seed):
    """Random shares that all carry one version-0 namespace (its id from the seed)."""
    s = synth.random_blob_square(k, seed).copy()
    s[:, :29] = np.frombuffer(bytes(19) + bytes([1 + seed % 200] * 10), np.uint8)
    return s


class Batch:
    """n squares extended on the device, their store, and per square the
    single-square reference: EDSAxisNodes, roots and the host's merkle proofs."""

    def __init__(self, ctx, k, seeds, one_namespace=False, reference=True):
        self.k, self.w, self.n = k, 2 * k, len(seeds)
        make = _one_namespace_square if one_namespace else synth.random_blob_square
        self.ods = [np.ascontiguousarray(make(k, s)) for s in seeds]
        self.ds = device.DeviceSquares(k, self.n, ctx=ctx)
        self.ds.load_ods(np.stack([o.reshape(-1) for o in self.ods]))
        self.ds.extend()
        torch.cuda.synchronize()
        assert (self.ds.status.cpu() == 0).all()
        self.store = self.ds.proof_store()
        self.roots = [[r.tobytes() for r in self.ds.row_roots[i].cpu().numpy()] +
                      [r.tobytes() for r in self.ds.col_roots[i].cpu().numpy()] for i in range(self.n)]
        self.data_roots = [self.ds.dah[i].cpu().numpy().tobytes() for i in range(self.n)]
        self.ref = [inclusion.EDSAxisNodes(k, self.ds.eds[i], ctx) for i in range(self.n)] if reference else None
        self._merkle = {}
        self.ctx = ctx

    def merkle(self, i):
        """proof.proofs_from_byte_slices(row_roots + col_roots) of square i."""
        if i not in self._merkle:
            self._merkle[i] = proof.proofs_from_byte_slices(self.roots[i], self.ctx)
        return self._merkle[i]

    def shares(self, i):
        return [self.ods[i][j].tobytes() for j in range(self.k * self.k)]


_batches = {}


def _batch(ctx, k, one_namespace=False):
    key = (k, one_namespace)
    if key not in _batches:
        _batches[key] = Batch(ctx, k, [7100 + k, 7200 + k, 7300 + k], one_namespace)
    return _batches[key]


def _regions(st):
    """The three regions of a store, without the alignment gaps between them."""
    return (st.store[:st.n * st.row_bytes], st.store[st.col_off:st.col_off + st.n * st.col_bytes],
            st.store[st.dah_off:st.dah_off + st.n * st.dah_bytes])


# ---- 1. the store equals the per-square stores ---------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_store_equals_per_square_stores(ctx, k):
    b = _batch(ctx, k)
    st, w = b.store, b.w
    L = ctx._L
    assert st.n == 3 and st.row_bytes == L.dagpu_row_nodes_size(k) and st.col_bytes == L.dagpu_col_nodes_size(k)
    assert st.col_off % 256 == 0 and st.dah_off % 256 == 0
    torch.cuda.synchronize()
    tree = st.dah_tree().cpu().numpy()
    assert tree.shape == (3, 8 * k - 1, 32)
    for i in range(3):
        s = st.square(i)
        assert torch.equal(s.nodes, b.ref[i].nodes), (k, i)
        assert torch.equal(s.col_inner, b.ref[i].col_inner), (k, i)
        assert torch.equal(s.eds, b.ref[i].eds) and torch.equal(s.col_roots(), b.ref[i].col_roots())
        # RFC-6962 over rowRoots || colRoots, level by level
        level = [hashlib.sha256(b"\x00" + r).digest() for r in b.roots[i]]
        assert len(level) == 4 * k
        off = 0
        while True:
            got = [tree[i, off + j].tobytes() for j in range(len(level))]
            assert got == level, (k, i, len(level))
            off += len(level)
            if len(level) == 1:
                break
            level = [hashlib.sha256(b"\x01" + level[2 * j] + level[2 * j + 1]).digest()
                     for j in range(len(level) // 2)]
        assert off == 8 * k - 1
        assert st.data_roots()[i].cpu().numpy().tobytes() == level[0] == b.data_roots[i]
    # the same squares square_stride apart, junk between them
    one = w * w * 512
    stride = one + 4096 + 16
    buf = torch.randint(0, 256, (3 * stride,), dtype=torch.uint8, device="cuda")
    for i in range(3):
        buf[i * stride:i * stride + one] = b.ds.eds[i]
    strided = device.ProofStore(k, buf, square_stride=stride, ctx=ctx)
    assert strided.n == 3 and (strided.col_off, strided.dah_off) == (st.col_off, st.dah_off)
    torch.cuda.synchronize()
    for x, y in zip(_regions(strided), _regions(st)):
        assert torch.equal(x, y), k
    assert torch.equal(strided.square(2).eds, b.ds.eds[2])


def test_store_arguments(ctx):
    b = _batch(ctx, 2)
    with pytest.raises(ValueError):
        device.ProofStore(2, b.ds.eds, square_stride=16 * 512 + 8, ctx=ctx)
    with pytest.raises(ValueError):
        device.ProofStore(2, b.ds.eds, square_stride=16 * 512 - 16, ctx=ctx)
    with pytest.raises(DAError):
        device.ProofStore(3, b.ds.eds, ctx=ctx)
    L = ctx._L
    ws = torch.empty(256, dtype=torch.uint8, device="cuda")
    st = torch.empty(b.store.store.numel(), dtype=torch.uint8, device="cuda")
    args = (b.ds.eds.data_ptr(), 16 * 512, st.data_ptr(), ws.data_ptr(), 0)
    assert L.dagpu_proof_store_device(ctx.handle, 2, 0, *args) == ERR_ARG
    assert L.dagpu_proof_store_device(ctx.handle, 2, 3, b.ds.eds.data_ptr() + 8, *args[1:]) == ERR_ARG
    assert L.dagpu_proof_store_device(ctx.handle, 2, 3, None, *args[1:]) == ERR_ARG


# ---- 2. the existing single-square calls on a slice ----------------------------------------

def test_existing_calls_on_a_slice(ctx):
    k = 4
    b = _batch(ctx, k)
    w = b.w
    s, ref = b.store.square(1), b.ref[1]
    reqs = [(a, i, st, en) for a in (0, 1) for i in (0, 3, w - 1) for st, en in ((0, 1), (2, 7), (5, w), (0, w))]
    assert proof.prove_ranges(s, reqs) == proof.prove_ranges(ref, reqs)
    got = device.nmt_prove_batch_device(s, reqs, eds=s.eds)
    want = device.nmt_prove_batch_device(ref, reqs, eds=ref.eds)
    for x, y in zip(got[:3], want[:3]):
        assert torch.equal(x, y)
    assert (got[3] == want[3]).all()
    shares = b.shares(1)
    nss = sorted({x[:29] for x in shares})
    qs = [nss[0], nss[len(nss) // 2], nss[-1], b"\xff" * 29, bytes(29), nss[3][:28] + bytes([nss[3][28] ^ 1])]
    assert proof.prove_namespaces(s, qs) == proof.prove_namespaces(ref, qs)
    r1, c1 = device.nmt_namespace_ranges_device(s, qs)
    r2, c2 = device.nmt_namespace_ranges_device(ref, qs)
    assert (r1 == r2).all() and (c1 == c2).all() and c1[0] > 0


# ---- 3. the producer across squares ---------------------------------------------------------

def _requests(k, n_sq, seed, count):
    """Shuffled over squares and both axes: single cells, whole axes, ranges
    ending at 2k and random ranges."""
    rng = random.Random(seed)
    w = 2 * k
    out = []
    for sq_ in range(n_sq):
        for axis in (0, 1):
            out.append((sq_, axis, rng.randrange(w), 0, w))                      # a whole axis
            out.append((sq_, axis, w - 1, w - 1, w))                             # the last cell
            out.append((sq_, axis, 0, 0, 1))                                     # the first cell
            out.append((sq_, axis, rng.randrange(w), rng.randrange(w), w))       # ending at 2k
    while len(out) < count:
        s = rng.randrange(w)
        e = s + 1 if rng.random() < 0.4 else rng.randrange(s + 1, w + 1)
        out.append((rng.randrange(n_sq), rng.randrange(2), rng.randrange(w), s, e))
    rng.shuffle(out)
    return out


def _check_against_single_square(b, reqs, out):
    """Nodes, namespaces, shares request by request against the single-square
    call of each square; aunts, leaf hash and axis root against the host."""
    torch.cuda.synchronize()
    k, w = b.k, b.w
    la = (4 * k).bit_length() - 1
    nodes, ns, cells = (t.cpu().numpy().tobytes() for t in (out.nodes, out.namespaces, out.shares))
    roots, hashes, aunts = (t.cpu().numpy().tobytes() for t in (out.axis_roots, out.leaf_hashes, out.aunts))
    assert len(roots) == 90 * len(reqs) and len(hashes) == 32 * len(reqs) and len(aunts) == 32 * la * len(reqs)
    for i in range(b.n):
        mine = [j for j, r in enumerate(reqs) if r[0] == i]
        if not mine:
            continue
        ref = device.nmt_prove_batch_device(b.ref[i], [reqs[j][1:] for j in mine], eds=b.ref[i].eds)
        torch.cuda.synchronize()
        rn, rs, rc = (t.cpu().numpy().tobytes() for t in ref[:3])
        _, merkle = b.merkle(i)
        for q, j in enumerate(mine):
            d, rd = out.desc[j], ref[3][q]
            assert tuple(d[:3]) == tuple(rd[:3]) == (reqs[j][3], reqs[j][4], reqs[j][4] - reqs[j][3])
            assert d[4] == rd[4] and d[6] == j and d[7] == j
            assert nodes[90 * d[5]:90 * (d[5] + d[4])] == rn[90 * rd[5]:90 * (rd[5] + rd[4])], (k, j, reqs[j])
            assert cells[512 * d[3]:512 * (d[3] + d[2])] == rc[512 * rd[3]:512 * (rd[3] + rd[2])], (k, j, reqs[j])
            assert ns[29 * j:29 * j + 29] == rs[29 * q:29 * q + 29]
            leaf = reqs[j][1] * w + reqs[j][2]
            mp = merkle[leaf]
            assert roots[90 * j:90 * j + 90] == b.roots[i][leaf], (k, j, reqs[j])
            assert hashes[32 * j:32 * j + 32] == mp.leaf_hash
            assert [aunts[32 * (j * la + a):32 * (j * la + a + 1)] for a in range(la)] == mp.aunts, (k, j, reqs[j])
            assert tuple(out.mdesc[j]) == (leaf, 4 * k, la, j * la, j, i)
    # the prefix sums leave no gaps
    assert out.desc[0][3] == 0 and out.desc[0][5] == 0
    assert (out.desc[1:, 3] == out.desc[:-1, 3] + out.desc[:-1, 2]).all()
    assert (out.desc[1:, 5] == out.desc[:-1, 5] + out.desc[:-1, 4]).all()
    assert out.nodes.numel() == 90 * int(out.desc[-1, 5] + out.desc[-1, 4])


def _merkle_status(ctx, b, out, aunts=None):
    """dagpu_merkle_verify_batch over mdesc: leaves = the emitted axis roots."""
    n = len(out.mdesc)
    lv = out.axis_roots.cpu().numpy()
    lh = out.leaf_hashes.cpu().numpy()
    au = out.aunts.cpu().numpy() if aunts is None else aunts
    rt = np.ascontiguousarray(b.store.data_roots().cpu().numpy())
    status = np.full(n, -99, np.int32)
    md = np.ascontiguousarray(out.mdesc)
    rc = ctx._L.dagpu_merkle_verify_batch(ctx.handle, n, _abi.addr(md), _abi.addr(lv), n, 90, _abi.addr(lh),
                                          _abi.addr(au), au.size // 32, _abi.addr(rt), b.n, _abi.addr(status))
    assert rc == OK
    return status


def _one_namespace(b, req):
    """VerifyInclusion prepends ONE namespace to every leaf: a produced proof
    verifies iff its cells share their namespace (Q0: the share's, else parity)."""
    i, axis, index, start, end = req
    k = b.k
    seen = set()
    for j in range(start, end):
        r, c = (index, j) if axis == 0 else (j, index)
        seen.add(b.ods[i][r * k + c, :29].tobytes() if r < k and c < k else b"\xff" * 29)
    return len(seen) == 1


@pytest.mark.parametrize("k", [1, 4, 8])
def test_producer_across_squares(ctx, k):
    b = _batch(ctx, k, one_namespace=True)
    reqs = _requests(k, 3, 90 + k, 60)
    out = device.nmt_prove_squares_device(b.store, reqs)
    _check_against_single_square(b, reqs, out)
    # round trip: the emitted roots table and the descriptors as they are
    want = np.array([OK if _one_namespace(b, r) else ERR_PROOF for r in reqs], np.int32)
    assert (want == OK).sum() >= len(reqs) // 2
    st = device.nmt_verify_batch_device(out.desc, out.namespaces, out.shares, 512, out.nodes, out.axis_roots, ctx=ctx)
    assert (st.cpu().numpy() == want).all()
    assert (_merkle_status(ctx, b, out) == OK).all()
    # one flipped byte in one aunt, and in one node, fails exactly that proof
    la = (4 * k).bit_length() - 1
    victim = len(reqs) // 2
    au = out.aunts.cpu().numpy().copy()
    au[32 * (victim * la + la - 1) + 5] ^= 0x40
    ms = _merkle_status(ctx, b, out, au)
    assert ms[victim] == ERR_PROOF and (np.delete(ms, victim) == OK).all()
    victim = next(j for j in range(len(reqs)) if out.desc[j][4] > 0 and want[j] == OK)
    bad = out.nodes.clone()
    bad[90 * int(out.desc[victim][5]) + 70] ^= 1
    st = device.nmt_verify_batch_device(out.desc, out.namespaces, out.shares, 512, bad, out.axis_roots,
                                        ctx=ctx).cpu().numpy()
    assert st[victim] == ERR_PROOF and (np.delete(st, victim) == np.delete(want, victim)).all()


def test_producer_optional_outputs(ctx):
    b = _batch(ctx, 4)
    reqs = _requests(4, 3, 5, 30)
    full = device.nmt_prove_squares_device(b.store, reqs)
    lean = device.nmt_prove_squares_device(b.store, reqs, shares=False, to_data_root=False)
    assert lean.shares is None and lean.axis_roots is None and lean.aunts is None and lean.mdesc is None
    assert torch.equal(lean.nodes, full.nodes) and torch.equal(lean.namespaces, full.namespaces)
    assert (lean.desc == full.desc).all()
    empty = device.nmt_prove_squares_device(b.store, np.zeros((0, 5), np.int64))
    assert empty.nodes.numel() == 0 and len(empty.desc) == 0


# ---- 4. ShareProofs --------------------------------------------------------------------------

def _share_ranges(k):
    kk = k * k
    out = [(0, 1), (1, k), (k - 1, k + 1), (0, kk), (kk - 1, kk)]
    if k >= 4:
        out += [(k + 2, 4 * k - 1), (1, 3 * k + 1)]
    return out


@pytest.mark.parametrize("k", [2, 4, 8])
def test_share_proofs_equal_new_share_inclusion_proof(ctx, k):
    b = _batch(ctx, k, one_namespace=True)
    ranges = [(i, s, e) for i in range(3) for s, e in _share_ranges(k)]
    random.Random(k).shuffle(ranges)
    got = b.ds.share_proofs(ranges)
    assert len(got) == len(ranges)
    for (i, s, e), p in zip(ranges, got):
        ns = b.ods[i][0, :29].tobytes()
        want = proof.new_share_inclusion_proof(b.shares(i), ns, (s, e), ctx)
        assert p.data == want.data, (k, i, s, e)
        assert p.share_proofs == want.share_proofs, (k, i, s, e)
        assert p.namespace_id == want.namespace_id and p.namespace_version == want.namespace_version
        assert p.row_proof == want.row_proof, (k, i, s, e)
        assert p == want
        p.validate(b.data_roots[i])
        with pytest.raises(DAError):
            p.validate(b.data_roots[(i + 1) % 3])
    roots = [b.data_roots[i] for i, _, _ in ranges]
    assert proof.validate_batch(got, roots, ctx) == [None] * len(got)
    wrong = proof.validate_batch(got, [b.data_roots[(i + 1) % 3] for i, _, _ in ranges], ctx)
    assert all(isinstance(x, DAError) for x in wrong)
    # explicit namespaces are taken as given
    other = bytes([0]) * 19 + bytes([9] * 10)
    assert b.ds.share_proofs(ranges[:2], namespaces=[other, other])[1].namespace_id == other[1:]
    assert b.ds.share_proofs([]) == []
    assert b.ds.proof_store() is b.store  # served from the cached store


def test_share_proofs_mixed_namespaces(ctx):
    k = 4
    b = _batch(ctx, k)  # random blob shares: (almost) every share its own namespace
    shares = b.shares(2)
    assert shares[0][:29] != shares[1][:29]
    with pytest.raises(DAError, match="different namespaces"):
        b.ds.share_proofs([(0, 0, 1), (2, 0, 2)])
    # one share has one namespace; with a namespace given the range is proven as asked
    one = b.ds.share_proofs([(2, 5, 6)])[0]
    assert one == proof.new_share_inclusion_proof(shares, shares[5][:29], (5, 6), ctx)
    ns = shares[0][:29]
    p = b.ds.share_proofs([(2, 0, 2 * k)], namespaces=[ns])[0]
    assert p == proof.new_share_inclusion_proof(shares, ns, (0, 2 * k), ctx)
    for bad in ((3, 0, 1), (0, 0, k * k + 1), (0, 2, 2), (-1, 0, 1)):
        with pytest.raises(DAError):
            b.ds.share_proofs([(0, 0, 1), bad])


# ---- 5. blob proofs ----------------------------------------------------------------------------

def test_blob_proofs(ctx):
    blocks, k = [], None
    for seed in range(40, 80):  # two small blocks of one width
        txs = synth.block_txs(2, 5, seed)
        kb, ods = sq.construct_native(txs)
        if k is None or kb == k:
            k = kb
            blocks.append((txs, ods))
        if len(blocks) == 2:
            break
    assert len(blocks) == 2 and k >= 2
    d = device.DeviceSquares(k, 2, ctx=ctx, in_place=True)
    d.load_txs([t for t, _ in blocks])
    d.extend()
    torch.cuda.synchronize()
    assert (d.status.cpu() == 0).all()
    rec, _ = d.blob_table()
    assert len(rec) == 10 and set(rec[:, 0]) == {0, 1}
    proofs = d.blob_proofs()
    roots = [d.dah[int(i)].cpu().numpy().tobytes() for i in rec[:, 0]]
    assert proof.validate_batch(proofs, roots, ctx) == [None] * len(proofs)
    for (i, first, count), p, root in zip(rec, proofs, roots):
        ods = np.asarray(blocks[int(i)][1]).reshape(k * k, 512)
        assert p.data == [ods[j].tobytes() for j in range(first, first + count)]
        assert bytes([p.namespace_version]) + p.namespace_id == ods[first, :29].tobytes()
        p.validate(root)
    some = d.blob_proofs(rows=[7, 2])
    assert some == [proofs[7], proofs[2]]
    # the cached store goes with the squares it was built from
    store = d.proof_store()
    assert d.proof_store() is store
    d.extend()
    assert d._proof_store is None and d.proof_store() is not store
    ods = np.stack([np.asarray(o).reshape(-1) for _, o in blocks])
    for drop in (lambda: d.load_txs([t for t, _ in blocks]), lambda: d.load_ods(ods)):
        assert d.proof_store() is d.proof_store()
        drop()
        assert d._proof_store is None


# ---- 6. refusals -------------------------------------------------------------------------------

def _raw(ctx, b, req, nodes_cap, shares_cap):
    """The C call with sentinel-filled outputs; returns (rc, everything it could write)."""
    n = len(req)
    la = (4 * b.k).bit_length() - 1
    dev = [torch.full((sz,), 0xA5, dtype=torch.uint8, device="cuda")
           for sz in (nodes_cap * 90 + 16, n * 29, shares_cap * 512 + 16, n * 90, n * 32, n * la * 32)]
    desc, mdesc = np.full((n, 8), -7, np.int64), np.full((n, 6), -7, np.int64)
    total = ctypes.c_size_t(12345)
    ws = torch.empty(ctx._L.dagpu_nmt_prove_squares_workspace_size(n), dtype=torch.uint8, device="cuda")
    r = np.ascontiguousarray(np.asarray(req, np.int64))
    rc = ctx._L.dagpu_nmt_prove_squares_device(
        ctx.handle, b.k, b.n, n, _abi.addr(r), b.store.eds.data_ptr(), b.store.square_stride,
        b.store.store.data_ptr(), dev[0].data_ptr(), nodes_cap, dev[1].data_ptr(), dev[2].data_ptr(), shares_cap,
        dev[3].data_ptr(), dev[4].data_ptr(), dev[5].data_ptr(), _abi.addr(desc), _abi.addr(mdesc),
        ctypes.byref(total), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, dev, desc, mdesc, total.value


def test_refusals_leave_everything_untouched(ctx):
    k = 4
    b = _batch(ctx, k)
    w = b.w
    good = _requests(k, 3, 17, 20)
    nodes_need = sum(bin(s).count("1") + 3 - bin(e - 1).count("1") for _, _, _, s, e in good)
    cells_need = sum(e - s for _, _, _, s, e in good)
    rc, dev, desc, mdesc, total = _raw(ctx, b, good, nodes_need, cells_need)
    assert rc == OK and total == nodes_need and (desc != -7).any() and (mdesc != -7).any()
    assert all((t.cpu() != 0xA5).any() for t in dev)

    def untouched(res):
        rc, dev, desc, mdesc, total = res
        assert rc == ERR_ARG
        assert all((t.cpu() == 0xA5).all() for t in dev) and (desc == -7).all() and (mdesc == -7).all()
        assert total == 12345

    for bad in ((3, 0, 0, 0, 1), (-1, 0, 0, 0, 1), (0, 2, 0, 0, 1), (0, -1, 0, 0, 1), (1, 0, w, 0, 1),
                (1, 1, -1, 0, 1), (2, 0, 0, -1, 1), (2, 0, 0, 3, 3), (2, 1, 0, 5, 4), (0, 0, 0, 0, w + 1)):
        reqs = good[:7] + [bad] + good[7:]
        untouched(_raw(ctx, b, reqs, nodes_need + 8, cells_need + 8))
        assert "request 7" in ctx.last_error()
        with pytest.raises(DAError):
            device.nmt_prove_squares_device(b.store, reqs)
    untouched(_raw(ctx, b, good, nodes_need - 1, cells_need))
    untouched(_raw(ctx, b, good, nodes_need, cells_need - 1))


# ---- 7. k = 128 ----------------------------------------------------------------------------------

def test_k128_two_squares(ctx):
    k = 128
    b = Batch(ctx, k, [9128, 9129], one_namespace=True)
    reqs = _requests(k, 2, 128, 300)
    out = device.nmt_prove_squares_device(b.store, reqs)
    _check_against_single_square(b, reqs, out)
    st = device.nmt_verify_batch_device(out.desc, out.namespaces, out.shares, 512, out.nodes, out.axis_roots, ctx=ctx)
    want = np.array([OK if _one_namespace(b, r) else ERR_PROOF for r in reqs], np.int32)
    assert (st.cpu().numpy() == want).all() and (want == OK).sum() >= 100
    assert (_merkle_status(ctx, b, out) == OK).all()
    for i in range(2):
        assert torch.equal(b.store.square(i).nodes, b.ref[i].nodes)
        assert torch.equal(b.store.square(i).col_inner, b.ref[i].col_inner)
        assert b.store.data_roots()[i].cpu().numpy().tobytes() == b.data_roots[i]
    kk = k * k
    ranges = [(0, 0, 1), (1, kk - 1, kk), (0, 100, 128), (1, 127, 129), (0, 300, 700), (1, 5 * k, 6 * k),
              (1, 0, 2 * k + 1), (0, kk - 3 * k - 7, kk), (1, 8191, 8193), (0, 16000, 16001), (1, 64, 65),
              (0, 129, 130 + k)]
    got = b.ds.share_proofs(ranges)
    shares = [b.shares(0), b.shares(1)]
    for (i, s, e), p in zip(ranges, got):
        assert p == proof.new_share_inclusion_proof(shares[i], shares[i][0][:29], (s, e), ctx), (i, s, e)
    assert proof.validate_batch(got, [b.data_roots[i] for i, _, _ in ranges], ctx) == [None] * len(got)
