"""The tx index on the host (csrc/square_units.hpp through
dagpu_square_units_host, the serial walk, and dagpu_square_units_emulate_host,
the device algorithm as a host loop; square.units_native): the unit table
against Builder.find_tx_share_range and the mirror's parse_txs, the boundary
streams, and the tampered and randomly mutated squares on which the parallel
walk must either agree with the serial one or hand the square to the host."""
import random
import struct

import numpy as np
import pytest

from celestia_da import _abi
from celestia_da import shares as sh
from celestia_da import square as sq

import square_read_cases as rc
import square_units_cases as cases

OK, HOST = _abi.UNITS_OK, _abi.UNITS_HOST


def both(shares, k=None):
    """(serial units, serial summary, emulated units, emulated summary) of one square."""
    ods = rc.ods_of(shares)
    _, rec, scan = sq.scan_native(ods, k)
    u, s = sq.units_native(ods, k, records=rec, scan=scan)
    eu, es = sq.units_native(ods, k, records=rec, scan=scan, emulate=True)
    return u, s, eu, es


@pytest.mark.parametrize("name", [c[0] for c in cases.squares()])
def test_table_matches_builder_and_mirror(name):
    _, k, shares, txs = next(c for c in cases.squares() if c[0] == name)
    want, data = cases.mirror_units(shares)
    u, s, eu, es = both(shares, k)
    n_tx = int((want["flags"] == _abi.SEQ_TX).sum())
    assert list(s) == [OK, 0, len(want), n_tx, len(want) - n_tx, sum(rc.up16(len(d)) for d in data), 0, 0]
    assert u.tobytes() == want.tobytes()
    # the device algorithm: never the host for a square the splitters made
    assert list(es) == list(s) and eu.tobytes() == u.tobytes()
    ods = rc.ods_of(shares)
    _, rec, _ = sq.scan_native(ods, k)
    assert [sq.unit_bytes(ods, k, k * 512, rec, r) for r in u] == data
    if txs is not None:
        b = sq.Builder(128, sq.LATEST_VERSION, *txs)
        b.export()
        if any(len(t) == 0 for t in txs):
            # parseRawData stops at a length of 0: the reference reads back no tx from an empty tx on
            # (parse_txs, the mirror's `data`), though the Builder counted them
            assert len(u) == len(data) < len(b.txs) + len(b.pfbs)
        else:
            assert len(u) == len(b.txs) + len(b.pfbs)
        for i, r in enumerate(u):
            rng = b.find_tx_share_range(i)
            assert (int(r["start_share"]), int(r["end_share"])) == (rng.start, rng.end), i
        assert data == sh.parse_txs(rc.compact_range(list(shares), sh.TX_NAMESPACE)) + \
            sh.parse_txs(rc.compact_range(list(shares), sh.PAY_FOR_BLOB_NAMESPACE))


def _units_of(name):
    _, k, shares, _ = next(c for c in cases.squares() if c[0] == name)
    return shares, cases.mirror_units(shares)[0]


def _reserved(share, j):
    return struct.unpack(">I", share.data[34:38] if j == 0 else share.data[30:34])[0]


def test_boundary_situations_occur():
    """Each situation the walk has to get right is really in the squares."""
    # a unit ending on a share's last byte: the next share's reserved value is 34
    shares, u = _units_of("unit_ends_with_share")
    ends = [int(r["offset"] + r["len"]) for r in u]
    assert 474 in ends and 952 in ends and _reserved(shares[1], 1) == 34 and _reserved(shares[2], 2) == 34
    # a 2-byte delimiter whose unit fills the rest of the share exactly
    assert int(u[0]["offset"]) == 2 and ends[0] == 474
    # a delimiter straddling two shares
    shares, u = _units_of("delimiter_straddles")
    straddle = [r for r in u if cases.share_of(int(r["offset"]) - 2) != cases.share_of(int(r["offset"]) - 1)
                and r["len"] >= 128]
    assert len(straddle) == 2
    # a unit spanning >= 3 shares: the middle shares have reserved bytes 0
    shares, u = _units_of("tx_5000")
    assert u[0]["end_share"] - u[0]["start_share"] >= 3
    assert all(_reserved(shares[j], j) == 0 for j in range(1, int(u[0]["end_share"]) - 1))
    # >= 200 one-byte txs in one share
    shares, u = _units_of("many_small_txs")
    assert np.bincount(u["start_share"]).max() >= 200 and set(u["len"]) == {1}
    # a sequence whose last unit ends on the last byte of its last share
    for name, payload in (("tx_fills_one_share", 474), ("tx_fills_two_shares", 952)):
        shares, u = _units_of(name)
        assert len(u) == 1 and int(u[0]["offset"] + u[0]["len"]) == payload
    # only PFBs, only txs
    _, u = _units_of("blob_478")
    assert len(u) >= 1 and set(u["flags"]) == {_abi.SEQ_PFB}
    _, u = _units_of("tx_957")
    assert len(u) == 1 and set(u["flags"]) == {_abi.SEQ_TX}
    # the tx sequence ends on a share boundary and PFBs follow
    shares, u = _units_of("txs_end_on_boundary_then_pfbs")
    assert [int(f) for f in u["flags"]] == [_abi.SEQ_TX, _abi.SEQ_PFB]
    assert int(u[0]["offset"] + u[0]["len"]) == 474 and (int(u[1]["start_share"]), int(u[1]["offset"])) == (1, 2)


def either_or(shares, k=4):
    """The emulation's verdict on a square that may be broken: UNITS_OK with the
    serial table, or UNITS_HOST.  Returns the code."""
    ods = rc.ods_of(shares)
    _, rec, scan = sq.scan_native(ods, k)
    assert scan[0] == _abi.SCAN_OK
    eu, es = sq.units_native(ods, k, records=rec, scan=scan, emulate=True)
    if es[0] == HOST:
        assert list(es[2:]) == [0] * 6 and 0 <= es[1] < k * k
        return HOST
    # OK: then the serial walk has no error and the same table
    u, s = sq.units_native(ods, k, records=rec, scan=scan)
    assert es[0] == OK and list(es) == list(s) and eu.tobytes() == u.tobytes()
    return OK


@pytest.mark.parametrize("name", [c[0] for c in cases.tampered()])
def test_tampered(name):
    _, shares, host = next(c for c in cases.tampered() if c[0] == name)
    assert either_or(shares) == (HOST if host else OK)


def test_tampered_serial_answers():
    """What the host executor, the authority, says where the device gives up."""
    t = {name: shares for name, shares, _ in cases.tampered()}
    base_units, _ = cases.mirror_units(cases.tamper_base())
    n_pfb = int((base_units["flags"] == _abi.SEQ_PFB).sum())
    # a first share that gives no data: the tx sequence has no units
    u, s = sq.units_native(rc.ods_of(t["first_reserved_zero"]), 4)
    assert list(s[:5]) == [OK, 0, n_pfb, 0, n_pfb]
    with pytest.raises(sq.ShareError, match="varint overflows a 64-bit integer"):
        sq.units_native(rc.ods_of(t["overflowing_varint_at_a_unit_start"]), 4)
    # the byte behind the last unit is one more unit of 5 bytes
    u, s = sq.units_native(rc.ods_of(t["byte_in_the_padding_behind_the_last_unit"]), 4)
    assert s[3] == 6 and int(u[5]["len"]) == 5 and int(u[5]["offset"]) == 2110
    # first reserved bytes outside the content: refused as dagpu_compact_units refuses them
    for r in (37, 512):
        bad = rc._patch(cases.tamper_base(), [(0, 34, cases.be(r))])
        with pytest.raises(ValueError, match=f"reserved bytes {r} point outside"):
            sq.units_native(rc.ods_of(bad), 4)
        assert either_or(bad) == HOST


def test_random_mutations():
    rng = random.Random(2000)
    bases = cases.mutation_bases()
    count = {OK: 0, HOST: 0}
    for _ in range(2000):
        shares = cases.mutate(rng, rng.choice(bases))
        try:
            count[either_or(shares, int(len(shares) ** 0.5))] += 1
        except (sq.ShareError, ValueError):
            # the serial walk has an error: the emulation said OK, which it must not
            raise AssertionError("UNITS_OK on a square the serial walk refuses")
    assert count[OK] > 0 and count[HOST] > 0 and count[OK] + count[HOST] == 2000


def test_overflow_and_scan_codes():
    shares, want = _units_of("many_small_txs")
    ods = rc.ods_of(shares)
    for emulate in (False, True):
        u, s = sq.units_native(ods, unit_cap=len(want) - 1, emulate=emulate)
        assert list(s[:3]) == [_abi.UNITS_OVERFLOW, len(want), len(want)] and u.tobytes() == want[:-1].tobytes()
    broken = rc.tampered()[0][1]
    for emulate in (False, True):
        u, s = sq.units_native(rc.ods_of(broken), 4, emulate=emulate)
        assert list(s) == [_abi.UNITS_SCAN, 0, 0, 0, 0, 0, 0, 0] and len(u) == 0
