"""Squares shared by the square-read tests (tests/test_square_read_host.py,
test_square_read_check.py on the CPU, test_gpu_square_read.py on the GPU) and
what the Python mirror says about them.  Every expected value here comes from
celestia_da.shares / celestia_da.square (the mirror, pinned to the reference's
tables by test_shares_host.py and test_square_host.py), never from the library
under test:

  accepted()      the blocks of square_corpus.corpus() that square.construct accepts
  hand_made()     k = 64 squares put together from split_blobs, compact
                  splitters and padding shares: sequences that start at shares
                  63, 64, 65, 1023, 1024 and 1025 (the edges of a wave and of a
                  1024-share scan workgroup), a blob of 1,100 shares that spans
                  two workgroups, a sequence that ends on the square's last share
  tampered()      k = 4 squares with one broken rule each, and the (code, index)
                  the rule implies
  mirror_records  parse_shares(square, False) as dagpu_seq_record values
"""
import functools
import random
import struct

import numpy as np

from celestia_da import _abi
from celestia_da import shares as sh
from celestia_da import square as sq

from square_corpus import corpus
from test_square_host import NS1, NS2, NS3, blob_txs, normal_txs

A = sh.available_bytes_from_sparse_shares


def ods_of(shares):
    return np.frombuffer(b"".join(s.to_bytes() for s in shares), np.uint8).copy()


def up16(v):
    return (v + 15) & ~15


def seq_payload(q):
    """What dagpu_square_read_device yields for a non-padding sequence: a
    blob's data, a compact sequence's raw data of every share, uncut."""
    if q.shares[0].is_compact_share():
        return b"".join(s.raw_data() for s in q.shares)
    return q.raw_data()


def mirror_records(shares):
    """(records, summary) the scan must produce for a square parse_shares
    accepts, from the mirror's own parse."""
    seqs = sh.parse_shares(shares, False)
    rec = np.zeros(len(seqs), sq.seq_dtype())
    at = nblob = blob_bytes = compact_bytes = 0
    for r, q in zip(rec, seqs):
        first = q.shares[0]
        ns = q.namespace
        cls = _abi.SEQ_TX if ns == sh.TX_NAMESPACE else _abi.SEQ_PFB if ns == sh.PAY_FOR_BLOB_NAMESPACE \
            else _abi.SEQ_SPARSE
        r["ns"][:29] = np.frombuffer(ns, np.uint8)
        r["first"], r["count"], r["seq_len"] = at, len(q.shares), q.sequence_len()
        r["flags"] = cls | (_abi.SEQ_PADDING if q.is_padding() else 0) | first.version() << _abi.SEQ_VERSION_SHIFT
        if first.is_compact_share():
            r["reserved"] = struct.unpack(">I", first.data[34:38])[0]
        r["payload"] = 0 if q.is_padding() else len(seq_payload(q))
        if not q.is_padding():
            if cls == _abi.SEQ_SPARSE:
                nblob, blob_bytes = nblob + 1, blob_bytes + up16(int(r["payload"]))
            else:
                compact_bytes += up16(int(r["payload"]))
        at += len(q.shares)
    versions = [i for i, s in enumerate(shares) if s.version() != 0]
    summary = np.array([0, 0, versions[0] if versions else -1, len(seqs), nblob, blob_bytes, compact_bytes, 0],
                       np.int32)
    return rec, summary


def blob_range(shares):
    """The shares parse_blobs is given: everything outside the tx and PFB namespaces."""
    return [s for s in shares if not s.is_compact_share()]


def compact_range(shares, ns):
    r = sh.get_share_range_for_namespace(shares, ns)
    return shares[r.start:r.end]


@functools.lru_cache(maxsize=None)
def accepted():
    """((name, txs, k, Square)) of the corpus blocks Construct accepts."""
    out = []
    for name, txs, m in corpus():
        try:
            s = sq.construct(txs, max_square_size=m)
        except sq.ShareError:
            continue
        out.append((name, txs, s.size(), s))
    return tuple(out)


def _blob(rng, ns, shares, cut=5):
    """A blob that takes exactly `shares` shares."""
    return sh.Blob.new(ns, rng.randbytes(A(shares) - (cut if A(shares) > cut else 0)))


def _ns(i):
    return sh.new_namespace_v0(bytes([i]) * 10)


@functools.lru_cache(maxsize=None)
def hand_made():
    """((name, k, shares, starts)): `starts` are first shares the square must have."""
    rng = random.Random(64)
    k, total = 64, 64 * 64
    # all blobs: starts at 0, 63, 64, 65, 1023, 1024, 1025 (1,100 shares, over the
    # workgroup edge at 2048), two namespace padding shares, the last blob ends
    # on share 4095
    w = sh.SparseShareSplitter()
    for i, n in enumerate((63, 1, 1, 1023 - 65, 1, 1, 1100)):
        w.write(_blob(rng, _ns(i + 1), n))
    assert w.count() == 2125
    w.write_namespace_padding_shares(2)
    w.write(_blob(rng, _ns(9), total - 2127, cut=0))
    a = list(w.export())
    assert len(a) == total
    # txs, PFB-namespace units, reserved padding, blobs with namespace padding
    # between them, tail padding: 63 tx shares, the PFB sequence starts at 63
    tw = sh.CompactShareSplitter(sh.TX_NAMESPACE)
    while tw.count() < 63:
        tw.write_tx(rng.randbytes(rng.choice([1, 90, 300])))  # a unit adds one share at most
    txs = list(tw.export())
    assert len(txs) == 63
    pw = sh.CompactShareSplitter(sh.PAY_FOR_BLOB_NAMESPACE)
    while pw.count() < 3:
        pw.write_tx(rng.randbytes(200))
    b = txs + list(pw.export())
    b += sh.reserved_padding_shares(1023 - len(b))
    bw = sh.SparseShareSplitter()
    bw.write(_blob(rng, NS1, 1))            # 1023
    bw.write(_blob(rng, NS1, 1, cut=0))     # 1024: its data ends with its share
    bw.write(_blob(rng, NS2, 1100))         # 1025
    bw.write_namespace_padding_shares(3)
    bw.write(_blob(rng, NS3, 2))
    b += list(bw.export())
    b += sh.tail_padding_shares(total - len(b))
    return (("blobs_to_the_last_share", k, tuple(a), (0, 63, 64, 65, 1023, 1024, 1025, 2125, 2126, 2127)),
            ("txs_pfbs_blobs_padding", k, tuple(b), (0, len(txs), 1023, 1024, 1025, 2125, 2128, total - 1)))


def _patch(shares, edits):
    out = [bytearray(s.to_bytes()) for s in shares]
    for share, at, val in edits:
        if isinstance(val, bytes):
            out[share][at:at + len(val)] = val
        else:
            out[share][at] = val
    return [sh.Share(bytes(x)) for x in out]


@functools.lru_cache(maxsize=None)
def tampered():
    """((name, shares, code, index, version_share)) at k = 4.  The base square
    has a tx share, the PFB shares and blobs of 3 and 2 shares."""
    rng = random.Random(4)
    base = sq.construct(normal_txs(rng, 1) + blob_txs([NS1, NS2], [[A(3) - 9], [A(2) - 9]], rng))
    assert base.size() == 4
    seqs = sh.parse_shares(base, False)
    firsts, at = [], 0
    for q in seqs:
        firsts.append(at)
        at += len(q.shares)
    blobs = [(f, len(q.shares)) for f, q in zip(firsts, seqs)
             if not q.is_padding() and not q.shares[0].is_compact_share()]
    (f, c), (g, d) = blobs
    assert (c, d) == (3, 2) and f < g
    info = base[f + 1].data[29]
    be = lambda v: struct.pack(">I", v)  # noqa: E731
    N, I, L, OK = _abi.SCAN_NAMESPACE, _abi.SCAN_INCONSISTENT, _abi.SCAN_LENGTH, _abi.SCAN_OK
    cases = [
        ("namespace_version", [(f, 0, 1)], N, f, -1),
        ("v0_namespace_prefix", [(g, 5, 1)], N, g, -1),
        ("first_share_is_continuation", [(0, 29, base[0].data[29] & 0xFE)], I, 0, -1),
        ("continuation_other_namespace", [(f + 1, 28, base[f + 1].data[28] ^ 1)], I, f + 1, -1),
        ("length_one_share_long", [(f, 30, be(A(c) + 1))], L, f, -1),
        ("length_one_share_short", [(f, 30, be(A(c - 1)))], L, f, -1),
        ("length_zero_then_continuation", [(f, 30, be(0))], L, f, -1),
        ("share_version_1", [(f + 1, 29, info | 2)], OK, 0, f + 1),
        ("two_errors_lower_wins", [(g, 0, 9), (f + 1, 28, base[f + 1].data[28] ^ 1)], I, f + 1, -1),
        ("namespace_and_inconsistent_same_share", [(f + 1, 0, 7)], N, f + 1, -1),
        ("pass1_behind_pass2", [(f, 30, be(A(c) + 1)), (g + 1, 0, 3)], N, g + 1, -1),
    ]
    return tuple((name, tuple(_patch(base, edits)), code, index, ver) for name, edits, code, index, ver in cases)


def mirror_error(shares):
    """The message parse_shares (then parse_blobs of the blob range) raises, or None."""
    try:
        sh.parse_shares(list(shares), False)
        sh.parse_blobs(blob_range(list(shares)))
    except sh.ShareError as e:
        return str(e)
    return None
