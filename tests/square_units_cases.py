"""Squares shared by the tx-index tests (tests/test_square_units_host.py,
test_square_units_check.py on the CPU, test_gpu_square_units.py on the GPU) and
what the Python mirror says about them.  Every expected value comes from
celestia_da.shares / celestia_da.square (the mirror), never from the library
under test:

  squares()       the accepted corpus blocks of square_read_cases, the boundary
                  blocks below and the hand-made k = 64 squares:
                  (name, k, shares, txs or None)
  BOUNDARY        blocks that put a unit's end or a delimiter on a share's edge
                  where the corpus does not
  mirror_units    the unit table parse_shares + parse_compact_shares imply, in
                  block tx order, with each unit's bytes
  tamper_base     a k = 4 square whose tx sequence has five shares: two units in
                  share 0, a unit that covers share 2 entirely, a delimiter that
                  straddles shares 3 | 4
  tampered()      that square with one broken rule each; `host` says whether
                  the device algorithm has to hand the square to the host
"""
import functools
import random
import struct

import numpy as np

from celestia_da import _abi
from celestia_da import shares as sh
from celestia_da import square as sq

import square_read_cases as rc
from test_square_host import NS1, blob_txs

_rng = random.Random(31)
BOUNDARY = (
    # 2 + 472 = 474 and 2 + 950 = 952 stream bytes: the only unit ends on the last
    # byte of the sequence's last share
    ("tx_fills_one_share", [_rng.randbytes(472)]),
    ("tx_fills_two_shares", [_rng.randbytes(950)]),
    # the tx sequence ends on a share boundary and PFBs follow
    ("txs_end_on_boundary_then_pfbs", [_rng.randbytes(472)] + blob_txs([NS1], [[100]], _rng)),
)


def share_of(p):
    return 0 if p < 474 else 1 + (p - 474) // 478


def mirror_units(shares):
    """(records, bytes): records a unit_dtype() array in block tx order (the tx
    namespace's units, then the PFB namespace's), bytes the units' data."""
    seqs = sh.parse_shares(list(shares), False)
    found = {_abi.SEQ_TX: [], _abi.SEQ_PFB: []}
    first = 0
    for q, seq in enumerate(seqs):
        ns = seq.namespace
        cls = _abi.SEQ_TX if ns == sh.TX_NAMESPACE else _abi.SEQ_PFB if ns == sh.PAY_FOR_BLOB_NAMESPACE else 0
        if cls and not seq.is_padding():
            data = rc.seq_payload(seq)
            at = struct.unpack(">I", seq.shares[0].data[34:38])[0] - 38
            for u in sh.parse_compact_shares(seq.shares):
                d = at
                at += sh.delim_len(len(u))
                assert data[at:at + len(u)] == u
                found[cls].append(((first + share_of(d), first + share_of(at + len(u) - 1) + 1, q, cls, at, len(u)), u))
                at += len(u)
        first += len(seq.shares)
    both = found[_abi.SEQ_TX] + found[_abi.SEQ_PFB]
    return np.array([r for r, _ in both], sq.unit_dtype()), [u for _, u in both]


@functools.lru_cache(maxsize=None)
def squares():
    out = [(name, k, tuple(s), tuple(txs)) for name, txs, k, s in rc.accepted()]
    for name, txs in BOUNDARY:
        s = sq.construct(txs)
        out.append((name, s.size(), tuple(s), tuple(txs)))
    out += [(name, k, tuple(s), None) for name, k, s, _ in rc.hand_made()]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def tamper_txs():
    rng = random.Random(5)
    return tuple([rng.randbytes(n) for n in (300, 300, 1200, 100, 200)] + blob_txs([NS1], [[100]], rng))


@functools.lru_cache(maxsize=None)
def tamper_base():
    s = sq.construct(tamper_txs())
    assert s.size() == 4
    units, _ = mirror_units(s)
    # delimiters at 0, 302, 604, 1806, 1907 | 1908; the data of unit 2 covers share 2 (952 .. 1430)
    assert [int(u["offset"]) for u in units[:5]] == [2, 304, 606, 1807, 1909]
    reserved = [struct.unpack(">I", s[j].data[34 if j == 0 else 30:38 if j == 0 else 34])[0] for j in range(5)]
    assert reserved == [38, 34 + 604 - 474, 0, 34 + 1806 - 1430, 0]
    return tuple(s)


def be(v):
    return struct.pack(">I", v)


@functools.lru_cache(maxsize=None)
def tampered():
    """((name, shares, host)): host is True where the device algorithm must
    answer UNITS_HOST; elsewhere it may answer OK with the serial table."""
    base = tamper_base()
    end = 1909 + 200  # the tx stream's last data byte + 1, in share 4 (1908 .. 2386)
    cases = [
        ("reserved_into_a_unit", [(1, 30, be(34 + 604 - 474 + 6))], True),
        ("reserved_on_a_covered_share", [(2, 30, be(100))], True),
        ("reserved_cleared_where_a_unit_starts", [(3, 30, be(0))], True),
        ("first_reserved_zero", [(0, 34, be(0))], True),
        ("first_reserved_100", [(0, 34, be(100))], True),
        ("overflowing_varint_at_a_unit_start", [(0, 38 + 302, b"\xff" * 10)], True),
        ("byte_in_the_padding_behind_the_last_unit", [(4, 34 + end - 1908, 5)], True),
        # not reached by either walk: both give the untouched table
        ("byte_deep_in_the_padding", [(4, 34 + end - 1908 + 40, 5)], False),
        ("byte_inside_a_unit", [(2, 200, base[2].data[200] ^ 0xFF)], False),
    ]
    return tuple((name, tuple(rc._patch(base, edits)), host) for name, edits, host in cases)


def mutation_bases():
    """Small squares for the random mutations: the tamper base and corpus
    squares of k <= 4 with a compact share."""
    out = [tamper_base()]
    for name, k, s, _ in squares():
        if k <= 4 and name in ("delimiter_straddles", "unit_ends_with_share", "many_small_txs", "tx_957",
                               "txs_end_on_boundary_then_pfbs", "blob_478"):
            out.append(s)
    assert len(out) >= 6
    return out


def mutate(rng, shares):
    """One byte of one compact share changed: a reserved byte, or a content byte."""
    compact = [i for i, s in enumerate(shares) if s.is_compact_share() and not s.is_padding()]
    i = rng.choice(compact)
    start = shares[i].is_sequence_start()
    r_at = 34 if start else 30
    if rng.random() < 0.5:
        at = r_at + rng.randrange(4)
        # mostly the low bytes, so that the value stays inside the share
        if rng.random() < 0.8:
            at = r_at + rng.choice((2, 3, 3, 3))
    else:
        at = rng.randrange(r_at + 4, 512)
    val = rng.randrange(256) if rng.random() < 0.7 else rng.choice((0, 1, 0x80, 0xFF))
    return rc._patch(shares, [(i, at, val)])
