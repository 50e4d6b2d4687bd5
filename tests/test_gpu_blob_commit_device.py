"""Share commitments computed from squares resident in HBM
(dagpu_blob_commitments_device, csrc/blob_commit.hip; device.blob_commitments_device,
DeviceSquares.check_commitments) against
  * dagpu_blob_commitments fed the same shares from host memory (pinned to the
    reference's golden commitment 3b9e78b6...), for ranges of one namespace;
  * a host nmt + RFC-6962 computation from oracle/pyref.py primitives for
    ranges of up to 191 shares, each leaf under its own namespace;
  * the generic forest (trees.nmt_roots, trees.merkle_roots) for long ranges
    over many namespaces.
Every size at which the mountain range changes shape, both addressings, the
corpus of tests/square_corpus.py, the compare and push-order status bits, the
refusals, and one full 128 x 128 block end to end."""
import collections

import numpy as np
import pytest
import torch

import pyref
from celestia_da import _abi, blobtx as bt, da, inclusion as inc, square as sq, trees
from celestia_da.device import DeviceSquares, blob_commitments_device, write_squares_device

from square_corpus import corpus, full_block

pytestmark = pytest.mark.gpu

GOLDEN = "3b9e78b6648ec1a241925b31da2ecb50bfc6f4ad552d3279928ca13ebeba8c2b"
NS1 = trees.namespace_v0(b"\x01" * 10)


@pytest.fixture(scope="module")
def ctx():
    c = da.Context(0)
    # the reference the tests below lean on is itself the reference's golden
    assert trees.create_commitment(NS1, b"\xff" * 3 * 512, ctx=c).hex() == GOLDEN
    yield c
    c.close()


def _square(k, seed, run, parity_tail=0):
    """(k*k, 512) random shares whose namespaces never decrease: a new random
    namespace every `run` shares (run = 0: one namespace for the whole square),
    the last parity_tail shares under the parity namespace."""
    rng = np.random.default_rng(seed)
    n = k * k
    s = rng.integers(0, 256, (n, 512), dtype=np.uint8)
    runs = 1 if run == 0 else -(-n // run)
    nss = sorted(b"\x00" + bytes(rng.integers(0, 256, 28, dtype=np.uint8)) for _ in range(runs))
    for i in range(n):
        s[i, :29] = np.frombuffer(nss[0 if run == 0 else i // run], np.uint8)
    if parity_tail:
        s[n - parity_tail:, :29] = 0xFF
    return s


def _ref_lib(ctx, ranges):
    """dagpu_blob_commitments over host copies of the ranges ((count, 512)
    arrays of one namespace each): (status, (n, 32) commitments)."""
    ns = np.concatenate([r[0, :29] for r in ranges])
    cnt = np.array([len(r) for r in ranges], np.uint32)
    data = np.ascontiguousarray(np.concatenate(ranges).reshape(-1))
    out = np.zeros((len(ranges), 32), np.uint8)
    rc = ctx._L.dagpu_blob_commitments(ctx.handle, len(ranges), _abi.addr(ns), _abi.addr(cnt), _abi.addr(data), 64,
                                       _abi.addr(out))
    return rc, out


def _sizes(count):
    return pyref.mmr_sizes(count, pyref.subtree_width(count, 64))


def _ref_py(r):
    """Host nmt + RFC-6962: every leaf is share[0:29] | share; nmt's order rule
    holds inside each subtree (ValueError otherwise)."""
    roots, at = [], 0
    for sz in _sizes(len(r)):
        roots.append(pyref.nmt_root_generic([x[:29].tobytes() + x.tobytes() for x in r[at:at + sz]], True))
        at += sz
    return pyref.rfc6962(roots)


def _ref_forest(ctx, r):
    """The generic forest: one nmt per subtree, then HashFromByteSlices."""
    subs, at = [], 0
    for sz in _sizes(len(r)):
        subs.append([x[:29].tobytes() + x.tobytes() for x in r[at:at + sz]])
        at += sz
    return trees.hash_from_byte_slices(trees.nmt_roots(subs, True, ctx), ctx)


def _run(ctx, k, recs, buf, stride, pitch, expected=None):
    c, st, sqs = blob_commitments_device(k, recs, buf, stride, pitch, expected=expected, ctx=ctx)
    torch.cuda.synchronize()
    return c.cpu().numpy(), st.cpu().numpy(), sqs.cpu().numpy()


def _packed(squares):
    return torch.from_numpy(np.ascontiguousarray(np.stack(squares)).reshape(-1)).cuda()


# counts at k = 16 with an unaligned first share each; all but the first two cross a row end
K16_RANGES = [(1, 15), (2, 15), (3, 30), (64, 5), (65, 7), (127, 33), (129, 100), (191, 61)]


def test_shapes_k16(ctx):
    """One call over two squares: square 0 of one namespace (reference: the host
    route, and pyref), square 1 with a new namespace every 5 shares and a parity
    tail (reference: pyref, each leaf under its own namespace)."""
    k = 16
    one, many = _square(k, 1, 0), _square(k, 2, 5, parity_tail=40)
    recs = [(0, f, c) for c, f in K16_RANGES] + [(1, f, c) for c, f in K16_RANGES] + [(1, 256 - 70, 70)]
    com, st, sqs = _run(ctx, k, recs, _packed([one, many]), k * k * 512, k * 512)
    assert (st == 0).all() and (sqs == 0).all()
    rc, want = _ref_lib(ctx, [one[f:f + c] for c, f in K16_RANGES])
    assert rc == 0
    for i, (sqr, f, c) in enumerate(recs):
        src = (one, many)[sqr][f:f + c]
        assert com[i].tobytes() == _ref_py(src), recs[i]
        if sqr == 0:
            assert (com[i] == want[i]).all(), recs[i]
    # the golden blob itself, as three resident shares
    g = np.frombuffer(b"".join(trees.split_blob(NS1, b"\xff" * 3 * 512)), np.uint8).reshape(-1, 512)
    pad = np.concatenate([g, np.zeros((4 - len(g), 512), np.uint8)])
    com, st, _ = _run(ctx, 2, [(0, 0, len(g))], _packed([pad]), 4 * 512, 2 * 512)
    assert com[0].tobytes().hex() == GOLDEN and st[0] == 0


@pytest.mark.parametrize("k,count,first", [(64, 2049, 3), (128, 4097, 77), (128, 16383, 1), (256, 16385, 300)])
def test_long_ranges(ctx, k, count, first):
    """Subtrees of 64, 128 and 256 leaves, 33 to 134 of them per blob: a square
    of one namespace against the host route, one of many namespaces (a new one
    every 37 shares, parity at the end) against the generic forest."""
    one, many = _square(k, count, 0), _square(k, count + 1, 37, parity_tail=k)
    assert first + count <= k * k
    recs = [(0, first, count), (1, first, count), (1, k * k - count, count)]
    com, st, sqs = _run(ctx, k, recs, _packed([one, many]), k * k * 512, k * 512)
    assert (st == 0).all() and (sqs == 0).all()
    rc, want = _ref_lib(ctx, [one[first:first + count]])
    assert rc == 0 and (com[0] == want[0]).all()
    assert com[1].tobytes() == _ref_forest(ctx, many[first:first + count])
    assert com[2].tobytes() == _ref_forest(ctx, many[k * k - count:])


def test_addressing_packed_and_q0(ctx):
    """n = 3 squares, the same ranges in the packed layout and in Q0 at the EDS
    pitch inside a buffer pre-filled with 0xA5: identical results, and no byte
    of either buffer changes."""
    k = 16
    squares = [_square(k, 10 + i, (0, 3, 11)[i], parity_tail=(0, 0, 9)[i]) for i in range(3)]
    recs = [(i, f, c) for i in range(3) for c, f in K16_RANGES]
    packed = _packed(squares)
    eds = torch.full((3, 2 * k, 2 * k * 512), 0xA5, dtype=torch.uint8, device="cuda")
    eds[:, :k, :k * 512] = packed.view(3, k, k * 512)
    before_p, before_e = packed.clone(), eds.clone()
    a = _run(ctx, k, recs, packed, k * k * 512, k * 512)
    b = _run(ctx, k, recs, eds.view(-1), 4 * k * k * 512, 2 * k * 512)
    assert (a[0] == b[0]).all() and (a[1] == 0).all() and (b[1] == 0).all() and a[2].shape == b[2].shape == (3,)
    assert torch.equal(packed, before_p) and torch.equal(eds, before_e)
    for i, (s, f, c) in enumerate(recs):
        assert a[0][i].tobytes() == _ref_py(squares[s][f:f + c]), recs[i]


@pytest.fixture(scope="module")
def by_width():
    """{k: [(name, txs, plan)]} of the corpus blocks Construct accepts."""
    groups = collections.defaultdict(list)
    for name, txs, m in corpus():
        try:
            k, plan = sq.plan_native(txs, m)
        except sq.ShareError:
            continue
        groups[k].append((name, txs, plan))
    return dict(groups)


def _parsed_blobs(txs):
    """{data offset in the packed txs: (namespace, data, share_version)}."""
    out, at = {}, 0
    for raw in txs:
        t, ok = bt.unmarshal_blob_tx(raw)
        if ok:
            for (off, _), b in zip(bt.blob_data_offsets(raw), t.blobs):
                out[at + off] = (b.namespace(), b.data, b.share_version)
        at += len(raw)
    return out


def test_corpus_by_width(ctx, by_width):
    """Every accepted corpus block, one call per width, ranges from plan_blobs
    on squares written by write_squares_device; commitments equal
    create_commitments of the parsed blobs, matched by data_off."""
    assert sorted(by_width) == [1, 2, 4, 8, 16, 32, 64]
    total = 0
    for k, blocks in sorted(by_width.items()):
        n = len(blocks)
        out = torch.empty((n * k * k * 512,), dtype=torch.uint8, device="cuda")
        write_squares_device(k, [b[2] for b in blocks], [b"".join(b[1]) for b in blocks], out, k * k * 512, k * 512,
                             ctx=ctx)
        recs, want = [], []
        for i, (name, txs, plan) in enumerate(blocks):
            parsed = _parsed_blobs(txs)
            for first, count, off, ln in sq.plan_blobs(plan).tolist():
                recs.append((i, first, count))
                want.append(parsed[off])
        com, st, sqs = _run(ctx, k, np.array(recs, np.int64).reshape(-1, 3), out, k * k * 512, k * 512)
        assert (st == 0).all() and (sqs == 0).all() and len(sqs) == n
        if recs:
            ref = trees.create_commitments(want, ctx=ctx)
            for i in range(len(recs)):
                assert com[i].tobytes() == ref[i], (k, blocks[recs[i][0]][0], recs[i])
        total += len(recs)
    assert total >= 100


def test_corpus_block_equals_get_commitment(ctx, by_width):
    k = 16
    name, txs, plan = max(by_width[k], key=lambda b: len(sq.plan_blobs(b[2])))
    table = sq.plan_blobs(plan)
    assert k >= 4 and len(table) >= 2
    d = DeviceSquares(k, 1, ctx=ctx, in_place=True)
    d.load_txs([txs])
    com, st, _ = d.check_commitments()
    d.extend()
    torch.cuda.synchronize()
    assert (st.cpu() == 0).all() and (d.status.cpu() == 0).all()
    eds = d.eds.cpu().numpy().reshape(2 * k, 2 * k, 512)
    dah = da.DataAvailabilityHeader([r.tobytes() for r in d.row_roots[0].cpu().numpy()],
                                    [r.tobytes() for r in d.col_roots[0].cpu().numpy()])
    cacher = inc.EDSSubTreeRootCacher(k, eds, ctx)
    for row, c in zip(table.tolist(), com.cpu().numpy()):
        assert c.tobytes() == inc.get_commitment(cacher, dah, row[0], row[1]), (name, row)


def test_compare_flags_exactly_the_mismatches(ctx):
    k, n = 16, 3
    squares = [_square(k, 20 + i, 0) for i in range(n)]
    recs = [(i, f, c) for i in range(n) for c, f in K16_RANGES[:6]]
    packed = _packed(squares)
    good, st, sqs = _run(ctx, k, recs, packed, k * k * 512, k * 512)
    com, st, sqs = _run(ctx, k, recs, packed, k * k * 512, k * 512, expected=good)
    assert (com == good).all() and (st == 0).all() and (sqs == 0).all()
    # one byte of one expected commitment (a blob of square 0), one byte of one
    # share of another blob in another square
    a, b = 4, 2 * 6 + 3
    assert recs[a][0] == 0 and recs[b][0] == 2
    expected = good.copy()
    expected[a, 31] ^= 0x01
    sq_b, first_b, count_b = recs[b]
    hit = first_b
    others = [i for i, (s, f, c) in enumerate(recs) if s == sq_b and f <= hit < f + c and i != b]
    assert not others  # no other range of that square holds the share
    packed[(sq_b * k * k + hit) * 512 + 300] ^= 0x80
    com, st, sqs = _run(ctx, k, recs, packed, k * k * 512, k * 512, expected=torch.from_numpy(expected).cuda())
    want_st = np.zeros(len(recs), np.int32)
    want_st[[a, b]] = _abi.COMMIT_MISMATCH
    assert (st == want_st).all()
    assert sqs.tolist() == [_abi.COMMIT_MISMATCH, 0, _abi.COMMIT_MISMATCH]
    keep = [i for i in range(len(recs)) if i != b]
    assert (com[keep] == good[keep]).all() and (com[b] != good[b]).any()
    # a host array for `expected` is uploaded by the wrapper
    st2 = _run(ctx, k, recs, packed, k * k * 512, k * 512, expected=expected)[1]
    assert (st2 == want_st).all()


def test_push_order(ctx):
    """Share 1 under a smaller namespace than share 0: a 66-share range has
    two-leaf subtrees and reports it (nmt ErrInvalidPushOrder); a 64-share
    range has one-leaf subtrees, reports nothing and commits to the leaves as
    they are."""
    k = 16
    s = _square(k, 30, 0)
    s[:, 28] = 9
    s[1, 28] = 7
    assert s[1, :29].tobytes() < s[0, :29].tobytes()
    recs = [(0, 0, 66), (0, 0, 64), (0, 2, 66), (0, 1, 65)]
    com, st, sqs = _run(ctx, k, recs, _packed([s]), k * k * 512, k * 512)
    assert st.tolist() == [_abi.COMMIT_PUSH_ORDER, 0, 0, 0] and sqs.tolist() == [_abi.COMMIT_PUSH_ORDER]
    assert com[1].tobytes() == _ref_py_unchecked(s[:64])
    assert com[2].tobytes() == _ref_py(s[2:68]) and com[3].tobytes() == _ref_py(s[1:66])
    with pytest.raises(ValueError, match="push order"):
        _ref_py(s[:66])
    # share 7 below share 6, in subtrees of four leaves (130 and 200 shares: w = 4)
    t = _square(k, 31, 0)
    t[:, 28] = 5
    t[7, 28] = 4
    recs = [(0, 0, 130),   # leaf 3 of subtree 1, below leaf 2: the right child of a pair
            (0, 5, 130),   # leaf 2 of subtree 0, below leaf 1: the left child of the next pair
            (0, 4, 200),   # leaf 3 of subtree 0
            (0, 8, 130),   # not in the range
            (0, 7, 130),   # leaf 0 of the first subtree: nothing before it
            (0, 3, 130)]   # leaf 0 of subtree 1: its predecessor is in another tree
    com, st, _ = _run(ctx, k, recs, _packed([t]), k * k * 512, k * 512)
    assert st.tolist() == [_abi.COMMIT_PUSH_ORDER] * 3 + [0] * 3
    for i in (3, 4, 5):
        assert com[i].tobytes() == _ref_py(t[recs[i][1]:recs[i][1] + recs[i][2]])


def _ref_py_unchecked(r):
    """_ref_py for one-leaf subtrees (no order to check)."""
    assert all(sz == 1 for sz in _sizes(len(r)))
    return pyref.rfc6962([pyref.nmt_leaf_generic(x[:29].tobytes() + x.tobytes()) for x in r])


def _raw_call(ctx, k, n, recs, buf, stride, pitch, outs, threshold=64, base_off=0):
    rec = np.ascontiguousarray(np.array(recs, np.int64).reshape(-1, 3))
    com, st, sqs = outs
    return ctx._L.dagpu_blob_commitments_device(
        ctx.handle, k, n, len(rec), _abi.addr(rec) if len(rec) else None, buf.data_ptr() + base_off, stride, pitch,
        threshold, _abi.addr(com), None, _abi.addr(st), _abi.addr(sqs), None,
        int(torch.cuda.current_stream().cuda_stream))


def test_refusals_enqueue_nothing(ctx):
    k, n = 16, 2
    buf = _packed([_square(k, 40, 0), _square(k, 41, 0)])
    stride, pitch = k * k * 512, k * 512

    def outs():
        return (torch.full((2 * 32,), 0xA5, dtype=torch.uint8, device="cuda"),
                torch.full((2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda"),
                torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda"))

    good = [(0, 3, 70), (1, 250, 6)]
    o = outs()
    assert _raw_call(ctx, k, n, good, buf, stride, pitch, o) == 0
    torch.cuda.synchronize()
    assert (o[1].cpu() == 0).all() and (o[2].cpu() == 0).all() and not (o[0].cpu() == 0xA5).all()
    cases = [
        ("k not a power of two", dict(k=12), None),
        ("threshold 0", dict(threshold=0), None),
        ("row_pitch below k*512", dict(pitch=pitch - 16), None),
        ("misaligned base", dict(base_off=8), None),
        ("misaligned stride", dict(stride=stride + 8), None),
        ("misaligned pitch", dict(pitch=pitch + 8), None),
        ("square past n", dict(recs=[good[0], (2, 0, 1)]), "blob 1"),
        ("square negative", dict(recs=[(-1, 0, 1), good[1]]), "blob 0"),
        ("count zero", dict(recs=[good[0], (1, 4, 0)]), "blob 1"),
        ("range past the square", dict(recs=[good[0], (1, 250, 7)]), "blob 1"),
        ("first negative", dict(recs=[(0, -1, 2), good[1]]), "blob 0"),
    ]
    for what, change, names in cases:
        o = outs()
        a = dict(k=k, recs=good, stride=stride, pitch=pitch, threshold=64, base_off=0)
        a.update(change)
        rc = _raw_call(ctx, a["k"], n, a["recs"], buf, a["stride"], a["pitch"], o, a["threshold"], a["base_off"])
        assert rc == _abi.ERR_ARG, what
        if names:
            assert names in ctx.last_error(), (what, ctx.last_error())
        torch.cuda.synchronize()
        assert (o[0].cpu() == 0xA5).all() and (o[1].cpu() == 0x5A5A5A5A).all() and \
            (o[2].cpu() == 0x5A5A5A5A).all(), what
    o = outs()
    assert _raw_call(ctx, 2048, n, good, buf, 2048 * 2048 * 512, 2048 * 512, o) == _abi.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (o[1].cpu() == 0x5A5A5A5A).all() and (o[2].cpu() == 0x5A5A5A5A).all()
    # no blobs: OK, and only the square status is written (zeroed)
    o = outs()
    assert _raw_call(ctx, k, n, [], buf, stride, pitch, o) == 0
    torch.cuda.synchronize()
    assert (o[2].cpu() == 0).all() and (o[0].cpu() == 0xA5).all() and (o[1].cpu() == 0x5A5A5A5A).all()
    assert ctx._L.dagpu_blob_commitments_device(None, k, n, 0, None, None, stride, pitch, 64, None, None, None, None,
                                                None, None) == _abi.ERR_ARG
    # the wrapper raises
    with pytest.raises(da.DAError, match="blob 0") as e:
        blob_commitments_device(k, [(0, 255, 2)], buf, stride, pitch, ctx=ctx)
    assert e.value.code == _abi.ERR_ARG
    # a caller workspace of the advertised size serves the largest table mix
    need = ctx._L.dagpu_blob_commitments_workspace_size(k, 2, 76)
    assert need >= 76 * 96 + 38 * 96 and need % 16 == 0


def test_full_block_end_to_end(ctx):
    """The one large case: txs -> Q0 in place -> commitments checked against the
    declared ones -> extend; every status 0 and the DAH of the host route."""
    txs = full_block()
    k, ods = sq.construct_native(txs)
    assert k == 128
    d = DeviceSquares(k, 1, ctx=ctx, in_place=True)
    d.load_txs([txs])
    recs, keys = d.blob_table()
    assert len(recs) == 2000 and (keys[:, 0] == 0).all()
    parsed = _parsed_blobs(txs)
    declared = np.frombuffer(b"".join(trees.create_commitments([parsed[int(o)] for o in keys[:, 1]], ctx=ctx)),
                             np.uint8).reshape(-1, 32).copy()
    com, st, sqs = d.check_commitments(declared)
    d.extend()
    torch.cuda.synchronize()
    assert (st.cpu() == 0).all() and (sqs.cpu() == 0).all() and (d.status.cpu() == 0).all()
    assert (com.cpu().numpy() == declared).all()
    ref = DeviceSquares(k, 1, ctx=ctx)
    ref.load_ods(ods.reshape(1, -1))
    ref.extend()
    torch.cuda.synchronize()
    assert torch.equal(d.dah.cpu(), ref.dah.cpu())
    # after extend() Q0 is unchanged: the same answer, and a wrong declaration is caught
    declared[1234, 0] ^= 0xFF
    _, st, sqs = d.check_commitments(declared)
    torch.cuda.synchronize()
    assert st.cpu().nonzero().flatten().tolist() == [1234] and sqs.cpu().tolist() == [_abi.COMMIT_MISMATCH]
