"""Square read on the host (csrc/square_read.hpp through dagpu_square_scan_host
and dagpu_compact_units; square.parse_native): records, summaries, blob
payloads, tx units and Deconstruct against the Python mirror (shares.parse_shares,
parse_blobs, parse_txs, square.deconstruct) for every accepted corpus block,
hand-made k = 64 squares and one tampered square per rule of the scan."""
import numpy as np
import pytest

from celestia_da import _abi
from celestia_da import shares as sh
from celestia_da import square as sq

import square_read_cases as cases
from test_square_host import pfb_blob_sizes


def check_against_mirror(parsed, shares):
    """Every field of every record, the summary, blobs and units."""
    shares = list(shares)
    rec, summary = cases.mirror_records(shares)
    assert (parsed.summary == summary).all(), (parsed.summary, summary)
    assert len(parsed.records) == len(rec)
    for name in ("ns", "first", "count", "seq_len", "flags", "reserved", "payload"):
        assert (parsed.records[name] == rec[name]).all(), name
    assert parsed.blobs() == sh.parse_blobs(cases.blob_range(shares))
    assert parsed.txs() == sh.parse_txs(cases.compact_range(shares, sh.TX_NAMESPACE))
    assert parsed.wrapped_pfbs() == sh.parse_txs(cases.compact_range(shares, sh.PAY_FOR_BLOB_NAMESPACE))


def test_corpus_records_blobs_units_and_deconstruct():
    blocks = cases.accepted()
    assert len(blocks) >= 40
    for name, txs, k, square in blocks:
        parsed = sq.parse_native(cases.ods_of(square))
        assert parsed.k == k and parsed.summary[0] == _abi.SCAN_OK, name
        check_against_mirror(parsed, square)
        want = sq.deconstruct(square, pfb_blob_sizes)
        assert parsed.deconstruct(pfb_blob_sizes) == want, name
        if name != "zero_length_tx":
            assert want == list(txs), name


def test_zero_length_tx_gives_no_txs():
    """Its first delimiter is 0 and the reference stops there."""
    (square,) = [s for name, _, _, s in cases.accepted() if name == "zero_length_tx"]
    assert sh.parse_txs(cases.compact_range(list(square), sh.TX_NAMESPACE)) == []
    parsed = sq.parse_native(list(square))
    assert parsed.txs() == [] and parsed.deconstruct(pfb_blob_sizes) == []


def test_shares_needed_agrees_at_one_shares_content():
    """CompactSharesNeeded / SparseSharesNeeded compare with <, sq_compact_shares
    / sq_sparse_shares with <= and <: the scan accepts exactly the counts the
    mirror's functions give around every content boundary."""
    for compact, first, cont in ((True, 474, 478), (False, 478, 482)):
        ns = sh.TX_NAMESPACE if compact else cases.NS1
        for n in (1, 2, 3):
            for length in (first + (n - 1) * cont + d for d in (-1, 0, 1)):
                need = sh.compact_shares_needed(length) if compact else sh.sparse_shares_needed(length)
                for count in (need - 1, need, need + 1):
                    if count < 1:
                        continue
                    b = sh.Builder(ns, 0, True)
                    b.write_sequence_len(length)
                    b.zero_pad_if_necessary()
                    run = [b.build()]
                    for _ in range(count - 1):
                        c = sh.Builder(ns, 0, False)
                        c.zero_pad_if_necessary()
                        run.append(c.build())
                    square = run + sh.tail_padding_shares(16 - len(run))
                    _, _, summary = sq.scan_native(cases.ods_of(square))
                    want = (_abi.SCAN_OK, 0) if count == need else (_abi.SCAN_LENGTH, 0)
                    assert tuple(summary[:2]) == want, (compact, length, count)
                    try:
                        sh.parse_shares(square, False)
                        accepted = True
                    except sh.ShareError:
                        accepted = False
                    assert accepted == (count == need), (compact, length, count)


@pytest.mark.parametrize("which", [0, 1])
def test_hand_made_squares(which):
    name, k, shares, starts = cases.hand_made()[which]
    parsed = sq.parse_native(cases.ods_of(shares), k)
    check_against_mirror(parsed, shares)
    assert set(starts) <= set(parsed.records["first"].tolist()), name
    assert parsed.records["count"].max() >= 1100
    last = parsed.records[-1]
    assert int(last["first"]) + int(last["count"]) == k * k


@pytest.mark.parametrize("case", cases.tampered(), ids=lambda c: c[0])
def test_tampered_squares(case):
    name, shares, code, index, version_share = case
    _, _, summary = sq.scan_native(cases.ods_of(shares))
    assert (int(summary[0]), int(summary[1]), int(summary[2])) == (code, index, version_share)
    want = cases.mirror_error(shares)
    assert want is not None
    parsed = sq.parse_native(cases.ods_of(shares))
    with pytest.raises(sh.ShareError) as e:
        parsed.blobs()
    assert str(e.value) == want
    with pytest.raises(sh.ShareError) as e:
        parsed.deconstruct(pfb_blob_sizes)
    if code != _abi.SCAN_OK:
        assert str(e.value) == want


def test_seq_cap_overflow():
    name, k, shares, _ = cases.hand_made()[0]
    rec, summary = cases.mirror_records(list(shares))
    n = len(rec)
    _, got, s = sq.scan_native(cases.ods_of(shares), k, seq_cap=n)
    assert s[0] == _abi.SCAN_OK and got.tobytes() == rec.tobytes()
    _, got, s = sq.scan_native(cases.ods_of(shares), k, seq_cap=n - 1)
    assert tuple(s[:2]) == (_abi.SCAN_OVERFLOW, n) and s[3] == n and got.tobytes() == rec[:n - 1].tobytes()


@pytest.mark.parametrize("name", ["delimiter_straddles", "unit_ends_with_share", "many_small_txs", "tx_5000"])
def test_compact_units_delimiter_cases(name):
    (square,) = [s for n, _, _, s in cases.accepted() if n == name]
    run = cases.compact_range(list(square), sh.TX_NAMESPACE)
    raw = b"".join(s.raw_data() for s in run)
    reserved = int.from_bytes(run[0].data[34:38], "big")
    want = sh._parse_raw_data(run[0].raw_data_using_reserved() + b"".join(s.raw_data() for s in run[1:]))
    assert sq.compact_units(raw, reserved) == want and len(want) >= 1
    if name == "many_small_txs":
        assert len(want) == 700 and len(run) > 1


def test_compact_units_edges():
    u = sq.compact_units
    assert u(b"\x01a\x02bc", 0) == []                       # reserved 0: no unit starts in the first share
    assert u(b"\x01a\x02bc", 38) == [b"a", b"bc"] == sh._parse_raw_data(b"\x01a\x02bc")
    assert u(b"xx\x01a\x00\x01b", 40) == [b"a"]             # a zero delimiter ends the walk
    assert u(b"\x01a\x05bc", 38) == [b"a"]                   # a unit longer than what is left
    assert u(b"\x81", 38) == sh._parse_raw_data(b"\x81") == []
    # a varint of more bytes than its value needs: the reference skips the canonical length
    data = b"\x82\x80\x00" + b"\x01z" * 3
    assert u(data, 38) == sh._parse_raw_data(data)
    with pytest.raises(sh.ShareError, match="varint overflows"):
        u(b"\xff" * 12, 38)
    with pytest.raises(sh.ShareError, match="varint overflows"):
        sh._parse_raw_data(b"\xff" * 12)
    with pytest.raises(ValueError, match="reserved bytes 20"):
        u(b"\x01a", 20)


def test_scan_host_argument_refusals():
    L = _abi.lib()
    ods = np.zeros(4 * 512, np.uint8)
    rec = np.zeros(4, sq.seq_dtype())
    summary = np.full(8, 77, np.int32)
    for k, stride, pitch, word in ((3, 3 * 3 * 512, 3 * 512, "power of two"), (2048, 0, 2048 * 512, "power of two"),
                                   (2, 2 * 2 * 512, 512, "row_pitch")):
        rc = L.dagpu_square_scan_host(k, 1, _abi.addr(ods), stride, pitch, 4, _abi.addr(rec), _abi.addr(summary))
        assert rc == _abi.ERR_ARG and word in L.dagpu_last_error(None).decode()
    assert (summary == 77).all()
