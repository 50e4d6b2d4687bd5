"""Squares resident in HBM read back into sequences, blobs and txs
(dagpu_square_scan_device, dagpu_square_read_device, csrc/square_read.hip;
device.scan_squares_device, read_sequences_device, DeviceSquares.scan /
read_blobs / read_txs / deconstruct) against the Python mirror
(tests/square_read_cases.py): the accepted corpus squares batched by width in
both layouts, hand-made k = 64 squares, one tampered square per rule, the
namespace filter and its overflow, a record table that is too small, a repaired
batch read from Q0 in place, one full 128 x 128 block, and the refusals."""
import collections

import numpy as np
import pytest
import torch

from celestia_da import _abi, da
from celestia_da import shares as sh
from celestia_da import square as sq
from celestia_da.device import DeviceSquares, read_sequences_device, scan_squares_device

import square_read_cases as cases
from square_corpus import full_block
from test_square_host import NS1, NS2, NS3, blob_txs, normal_txs, pfb_blob_sizes  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
BOTH = _abi.READ_BLOBS | _abi.READ_COMPACT


@pytest.fixture(scope="module")
def ctx():
    c = da.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def expected():
    """{id(shares): (records, summary, [payload of every non-padding sequence])} from the mirror, once."""
    memo = {}

    def get(shares):
        key = id(shares)
        if key not in memo:
            rec, summary = cases.mirror_records(list(shares))
            pay = [cases.seq_payload(q) for q in sh.parse_shares(list(shares), False) if not q.is_padding()]
            memo[key] = (rec, summary, pay)
        return memo[key]
    return get


def place(k, squares, in_place):
    """n squares on the device: packed, or Q0 of a sentinel-filled EDS batch.
    Returns (flat tensor, square_stride, row_pitch, host copy)."""
    n = len(squares)
    ods = np.stack([cases.ods_of(s) for s in squares]).reshape(n, k, k * 512)
    if not in_place:
        host = ods.reshape(-1).copy()
        return torch.from_numpy(host).cuda(), k * k * 512, k * 512, host
    w = 2 * k
    host = np.full((n, w, w * 512), SENTINEL, np.uint8)
    host[:, :k, :k * 512] = ods
    host = host.reshape(-1)
    return torch.from_numpy(host.copy()).cuda(), w * w * 512, w * 512, host


def scan_and_read(ctx, k, squares, in_place, expected, namespaces=None, classes=BOTH):
    """Scan + read of n squares, every output checked against the mirror."""
    n = len(squares)
    buf, stride, pitch, host = place(k, squares, in_place)
    records, summary, shost = scan_squares_device(k, buf, stride, pitch, ctx=ctx)
    assert (summary.cpu().numpy() == shost).all()
    rec = records.cpu().numpy().view(sq.seq_dtype()).reshape(n, k * k)
    want_sel, want_pay = [], []
    for i, s in enumerate(squares):
        wrec, wsum, wpay = expected(s)
        assert (shost[i] == wsum).all(), (i, shost[i], wsum)
        assert rec[i, :len(wrec)].tobytes() == wrec.tobytes(), i
        live = [j for j in range(len(wrec)) if not wrec["flags"][j] & _abi.SEQ_PADDING]
        for j, p in zip(live, wpay):
            sparse = bool(wrec["flags"][j] & _abi.SEQ_SPARSE)
            if not classes & (_abi.READ_BLOBS if sparse else _abi.READ_COMPACT):
                continue
            if namespaces is not None and wrec["ns"][j][:29].tobytes() not in namespaces:
                continue
            want_sel.append(i * k * k + j)
            want_pay.append(p)
    need = sum(cases.up16(len(p)) for p in want_pay)
    assert need <= int(shost[:, 5].sum() + shost[:, 6].sum())
    payload = torch.full((need + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    selected, offsets, totals, _ = read_sequences_device(k, buf, stride, pitch, records, summary, need,
                                                         namespaces=namespaces, classes=classes, ctx=ctx,
                                                         payload=payload)
    torch.cuda.synchronize()
    assert totals.cpu().tolist() == [len(want_sel), need, 0]
    assert selected[:len(want_sel)].cpu().tolist() == want_sel
    got, at = payload.cpu().numpy(), 0
    offs = offsets[:len(want_sel)].cpu().tolist()
    for off, p in zip(offs, want_pay):
        assert off == at and off % 16 == 0
        assert got[off:off + len(p)].tobytes() == p
        at += cases.up16(len(p))
        assert (got[off + len(p):at] == SENTINEL).all()  # the gap to the next payload is not written
    assert (got[at:] == SENTINEL).all()
    assert (buf.cpu().numpy() == host).all()  # the squares, and the bytes around Q0, are as they were
    return shost


@pytest.fixture(scope="module")
def by_width():
    groups = collections.defaultdict(list)
    for name, _, k, s in cases.accepted():
        groups[k].append(s)
    return dict(groups)


@pytest.mark.parametrize("in_place", [False, True], ids=["packed", "q0_in_place"])
def test_corpus_batched_by_width(ctx, by_width, expected, in_place):
    assert {1, 2, 4, 8, 16} <= set(by_width)
    for k, squares in sorted(by_width.items()):
        for at in range(0, len(squares), 3):
            batch = [squares[(at + i) % len(squares)] for i in range(3)]
            scan_and_read(ctx, k, batch, in_place, expected)


@pytest.mark.parametrize("in_place", [False, True], ids=["packed", "q0_in_place"])
def test_hand_made_squares(ctx, expected, in_place):
    squares = [s for _, _, s, _ in cases.hand_made()]
    scan_and_read(ctx, 64, squares, in_place, expected)
    scan_and_read(ctx, 64, squares[::-1], in_place, expected, classes=_abi.READ_BLOBS)


def test_tampered_squares(ctx, expected):
    table = cases.tampered()
    good = cases.accepted()
    base = [s for _, _, k, s in good if k == 4][0]
    squares = [list(t[1]) for t in table] + [list(base)]
    n = len(squares)
    d = DeviceSquares(4, n, ctx=ctx)
    d.load_ods(np.stack([cases.ods_of(s) for s in squares]))
    host = d.scan(check=False)
    for i, (name, _, code, index, ver) in enumerate(table):
        assert (int(host[i, 0]), int(host[i, 1]), int(host[i, 2])) == (code, index, ver), name
    assert (host[n - 1] == expected(base)[1]).all()
    # the lowest bad square's message is the mirror's
    with pytest.raises(sh.ShareError) as e:
        d.scan()
    assert str(e.value) == cases.mirror_error(table[0][1])
    parsed = d._parsed(BOTH)
    for p, (name, shares, code, _, _) in zip(parsed, table):
        with pytest.raises(sh.ShareError) as e:
            p.blobs()
        assert str(e.value) == cases.mirror_error(shares), name
    assert parsed[-1].blobs() == sh.parse_blobs(cases.blob_range(list(base)))
    # squares whose code is not OK are not selected: only the last square's sequences and the version-1 square's
    records, summary, _, where = d._scan
    _, _, totals, _ = read_sequences_device(4, where[0], where[1], where[2], records, summary, 1 << 16, ctx=ctx)
    ok = [i for i in range(n) if host[i, 0] == _abi.SCAN_OK]
    assert len(ok) == 2
    want = sum(1 for i in ok for q in sh.parse_shares(squares[i], False) if not q.is_padding())
    assert totals.cpu().tolist()[0] == want


@pytest.fixture(scope="module")
def filter_square():
    """NS2 as three blobs with a namespace padding share between them (blobs of
    more than 64 shares start at even shares), NS1 and NS3 around."""
    import random
    r = random.Random(3)
    A = sh.available_bytes_from_sparse_shares
    txs = normal_txs(r, 3) + blob_txs([NS1, NS2, NS2, NS2, NS3], [[A(2)], [A(70) - 3, A(3) - 1, A(66)], [A(1)]], r)
    s = sq.construct(txs)
    seqs = sh.parse_shares(s, False)
    ns2 = [q for q in seqs if q.namespace == NS2]
    assert sum(not q.is_padding() for q in ns2) == 3 and any(q.is_padding() for q in ns2)
    return s.size(), s


def test_namespace_filter(ctx, expected, filter_square):
    k, s = filter_square
    absent = sh.new_namespace_v0(b"\x07" * 10)
    other = [x for _, _, kk, x in cases.accepted() if kk == k][:1]
    batch = [s] + other + [s]
    scan_and_read(ctx, k, batch, False, expected, namespaces=[NS2])
    scan_and_read(ctx, k, batch, True, expected, namespaces=[NS2, absent, NS3], classes=_abi.READ_BLOBS)
    scan_and_read(ctx, k, batch, False, expected, namespaces=[absent])
    scan_and_read(ctx, k, batch, False, expected, namespaces=[sh.TX_NAMESPACE])
    scan_and_read(ctx, k, batch, True, expected, namespaces=[sh.TX_NAMESPACE, NS2], classes=_abi.READ_COMPACT)


def test_payload_cap_one_byte_short(ctx, expected, filter_square):
    k, s = filter_square
    buf, stride, pitch, _ = place(k, [s, s], False)
    records, summary, _ = scan_squares_device(k, buf, stride, pitch, ctx=ctx)
    pays = [cases.seq_payload(q) for q in sh.parse_shares(list(s), False)
            if q.namespace == NS2 and not q.is_padding()] * 2
    offs = np.cumsum([0] + [cases.up16(len(p)) for p in pays])
    cap = int(offs[-2]) + len(pays[-1]) - 1
    payload = torch.full((int(offs[-1]) + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    _, offsets, totals, _ = read_sequences_device(k, buf, stride, pitch, records, summary, cap, namespaces=[NS2],
                                                  classes=_abi.READ_BLOBS, ctx=ctx, payload=payload)
    torch.cuda.synchronize()
    assert totals.cpu().tolist() == [len(pays), int(offs[-1]), 1]
    assert offsets[:len(pays)].cpu().tolist() == offs[:-1].tolist()
    got = payload.cpu().numpy()
    for off, p in zip(offs[:-2], pays[:-1]):
        assert got[off:off + len(p)].tobytes() == p
    assert (got[offs[-2]:] == SENTINEL).all()  # the sequence that does not fit is not written
    # with the one byte it fits
    _, _, totals, _ = read_sequences_device(k, buf, stride, pitch, records, summary, cap + 1, namespaces=[NS2],
                                            classes=_abi.READ_BLOBS, ctx=ctx, payload=payload)
    torch.cuda.synchronize()
    assert totals.cpu().tolist()[2] == 0
    assert payload.cpu().numpy()[offs[-2]:offs[-2] + len(pays[-1])].tobytes() == pays[-1]


def test_seq_cap_below_the_sequence_count(ctx, expected, by_width):
    k = 16
    squares = sorted(by_width[k], key=lambda s: len(expected(s)[0]))
    small, big = squares[0], squares[-1]
    cap = len(expected(big)[0]) - 1
    assert len(expected(small)[0]) <= cap
    batch = [small, big, small]
    buf, stride, pitch, _ = place(k, batch, False)
    records, summary, host = scan_squares_device(k, buf, stride, pitch, seq_cap=cap, ctx=ctx)
    assert host[:, 0].tolist() == [_abi.SCAN_OK, _abi.SCAN_OVERFLOW, _abi.SCAN_OK]
    assert int(host[1, 1]) == cap + 1 == int(host[1, 3])
    rec = records.cpu().numpy().view(sq.seq_dtype()).reshape(3, cap)
    for i, s in enumerate(batch):
        w = expected(s)[0][:cap]
        assert rec[i, :len(w)].tobytes() == w.tobytes()
    # the overflowed square is not selected
    selected, _, totals, _ = read_sequences_device(k, buf, stride, pitch, records, summary, 1 << 20, ctx=ctx)
    per = len(expected(small)[2])
    assert totals.cpu().tolist()[0] == 2 * per
    assert {int(x) // cap for x in selected[:2 * per].cpu().tolist()} == {0, 2}


def test_device_squares_repaired_q0(ctx):
    """load_txs -> extend -> erase three quarters of the cells -> repair ->
    read_blobs() and deconstruct() from Q0 in place."""
    import random
    k, r = 8, random.Random(8)
    A = sh.available_bytes_from_sparse_shares
    blocks = [normal_txs(r, 2 + i) + blob_txs([NS1, NS2, NS2], [[A(4 + i)], [A(9), A(2) - 1]], r) for i in range(3)]
    for b in blocks:
        assert sq.construct(b).size() == k
    n, w = len(blocks), 2 * k
    d = DeviceSquares(k, n, ctx=ctx, in_place=True)
    d.load_txs(blocks)
    d.extend()
    present = torch.zeros((n, w, w), dtype=torch.uint8, device="cuda")
    present[:, k:, k:] = 1  # only Q3 stays
    d.eds.copy_((d.eds.view(n, w * w, 512) * present.view(n, w * w, 1)).view(n, -1))
    status = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    present = present.view(n, -1).contiguous()
    d.repair(present, status, d.repair_workspace())
    torch.cuda.synchronize()
    assert (status.cpu() == 0).all()
    blobs = d.read_blobs()
    for b, txs in zip(blobs, blocks):
        assert b == sh.parse_blobs(cases.blob_range(list(sq.construct(txs))))
    assert d.deconstruct(pfb_blob_sizes) == [list(b) for b in blocks]
    assert sq.deconstruct_device(d, pfb_blob_sizes) == [list(b) for b in blocks]
    only = d.read_blobs(namespaces=[NS2])
    assert [len(x) for x in only] == [2] * n and all(x.namespace() == NS2 for y in only for x in y)
    txs, pfbs = zip(*d.read_txs())
    for i, b in enumerate(blocks):
        assert list(txs[i]) == b[:2 + i] and len(pfbs[i]) == 2


def test_full_block(ctx):
    """The one large case: 2,000 normal + 2,000 blob txs, k = 128."""
    txs = full_block()
    d = DeviceSquares(128, 1, ctx=ctx)
    d.load_txs([txs])
    host = d.scan()
    assert host[0, 0] == _abi.SCAN_OK and host[0, 4] == 2000
    assert d.deconstruct(pfb_blob_sizes) == [list(txs)]


def test_argument_refusals(ctx):
    k, n = 4, 2
    L = ctx._L
    buf = torch.zeros((n * k * k * 512 + 64,), dtype=torch.uint8, device="cuda")
    records = torch.full((n, k * k, 64), SENTINEL, dtype=torch.uint8, device="cuda")
    summary = torch.full((n, 8), 77, dtype=torch.int32, device="cuda")
    stride, pitch = k * k * 512, k * 512

    def scan(kk=k, base=0, st=stride, pt=pitch, rec=records, nn=n):
        return L.dagpu_square_scan_device(ctx.handle, kk, nn, buf.data_ptr() + base, st, pt, k * k, _abi.addr(rec),
                                          _abi.addr(summary), None, None, 0)

    for call, word in ((lambda: scan(kk=3), "power of two"), (lambda: scan(kk=2048), "power of two"),
                       (lambda: scan(base=8), "multiples of 16"), (lambda: scan(pt=pitch + 8), "multiples of 16"),
                       (lambda: scan(pt=pitch - 512), "row_pitch below"),
                       (lambda: scan(st=stride - 16), "square_stride below"),
                       (lambda: scan(nn=70000), "65535")):
        assert call() == _abi.ERR_ARG and word in ctx.last_error(), word
    selected = torch.full((n * k * k,), -7, dtype=torch.int32, device="cuda")
    offsets = torch.full((n * k * k,), -7, dtype=torch.int64, device="cuda")
    totals = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    payload = torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda")

    def read(kk=k, mask=BOTH, pay=payload.data_ptr(), ns=None, n_ns=0, sel=selected.data_ptr()):
        return L.dagpu_square_read_device(ctx.handle, kk, n, buf.data_ptr(), stride, pitch, k * k, _abi.addr(records),
                                          _abi.addr(summary), ns, n_ns, mask, sel, _abi.addr(offsets),
                                          _abi.addr(totals), pay, 4096, None, 0)

    for call, word in ((lambda: read(kk=5), "power of two"), (lambda: read(mask=0), "class_mask"),
                       (lambda: read(mask=4), "class_mask"),
                       (lambda: read(pay=payload.data_ptr() + 8), "multiples of 16"),
                       (lambda: read(n_ns=1), "null argument"), (lambda: read(sel=None), "null argument")):
        assert call() == _abi.ERR_ARG and word in ctx.last_error(), word
    torch.cuda.synchronize()
    assert (records.cpu() == SENTINEL).all() and (summary.cpu() == 77).all() and (payload.cpu() == SENTINEL).all()
    assert (selected.cpu() == -7).all() and (offsets.cpu() == -7).all() and (totals.cpu() == -7).all()
