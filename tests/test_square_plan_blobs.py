"""The blob table of a square plan (dagpu_square_plan_blobs, square.plan_blobs)
and the declared commitments in plan order (square.expected_commitments), on
the CPU: for every corpus block that Construct accepts the table is compared
with the blobs parsed from the txs and with the host-constructed square."""
import hashlib
import random

import numpy as np
import pytest

from celestia_da import blobtx as bt
from celestia_da import shares as sh
from celestia_da import square as sq

from square_corpus import corpus


def _blobs_by_offset(txs):
    """{offset of the data in the packed txs: Blob} over every BlobTx."""
    out, at = {}, 0
    for raw in txs:
        t, ok = bt.unmarshal_blob_tx(raw)
        if ok:
            for (off, ln), b in zip(bt.blob_data_offsets(raw), t.blobs):
                assert raw[off:off + ln] == b.data
                out[at + off] = b
        at += len(raw)
    return out


def test_plan_blobs_over_the_corpus():
    seen_blobs = seen_blocks = 0
    for name, txs, m in corpus():
        try:
            k, ods = sq.construct_native(txs, m)
        except sq.ShareError:
            continue
        pk, plan = sq.plan_native(txs, m)
        table = sq.plan_blobs(plan)
        assert pk == k and table.dtype == np.uint32 and table.shape[1:] == (4,), name
        want = _blobs_by_offset(txs)
        assert len(table) == len(want), name
        packed = b"".join(txs)
        shares = ods.reshape(k * k, 512)
        end = 0
        for first, count, off, ln in table.tolist():
            assert first >= end, name  # ascending, no overlap
            end = first + count
            b = want.pop(off)  # every blob once
            assert ln == len(b.data) and packed[off:off + ln] == b.data, name
            assert count == sh.sparse_shares_needed(ln), name
            s = shares[first].tobytes()
            assert s[:29] == b.namespace() and s[29] == 1 and int.from_bytes(s[30:34], "big") == ln, name
            for j in range(1, count):  # continuation shares of the same blob
                c = shares[first + j].tobytes()
                assert c[:29] == b.namespace() and c[29] == 0, (name, j)
        assert not want and end <= k * k, name
        seen_blobs += len(table)
        seen_blocks += 1
    assert seen_blocks >= 40 and seen_blobs >= 100


def _pfb_block(rng, mutate=None):
    """Three BlobTxs with real MsgPayForBlobs; namespaces out of order so that
    plan order differs from tx order.  Returns (txs, {data: commitment})."""
    nss = [sh.new_namespace_v0(bytes([v]) * 10) for v in (9, 3, 7, 3, 1)]
    groups = [[(nss[0], 700), (nss[1], 40000)], [(nss[2], 1)], [(nss[3], 478), (nss[4], 5000)]]
    txs, declared = [rng.randbytes(120), rng.randbytes(900)], {}
    for gi, group in enumerate(groups):
        blobs = [sh.Blob.new(ns, rng.randbytes(n)) for ns, n in group]
        msg = bt.MsgPayForBlobs(signer="celestia1signer", namespaces=[b.namespace() for b in blobs],
                                blob_sizes=[len(b.data) for b in blobs],
                                share_commitments=[hashlib.sha256(b.data).digest() for b in blobs],
                                share_versions=[0] * len(blobs))
        for b in blobs:
            declared[b.data] = hashlib.sha256(b.data).digest()
        if mutate:
            mutate(gi, msg)
        txs.append(bt.marshal_blob_tx(bt.marshal_sdk_tx(bt.URL_MSG_PAY_FOR_BLOBS, msg.marshal(), b"auth", [b"sig"]),
                                      *blobs))
    return txs, declared


def test_expected_commitments_in_plan_order():
    txs, declared = _pfb_block(random.Random(5))
    k, plan = sq.plan_native(txs)
    table = sq.plan_blobs(plan)
    got = sq.expected_commitments(txs, plan)
    assert got.shape == (5, 32) and got.dtype == np.uint8
    packed = b"".join(txs)
    order = []
    for row, c in zip(table.tolist(), got):
        data = packed[row[2]:row[2] + row[3]]
        assert c.tobytes() == declared[data]
        order.append(len(data))
    # sorted by namespace (1, 3, 3, 7, 9), blobs of one namespace in tx order: not the tx order
    assert order == [5000, 40000, 478, 1, 700]


def test_expected_commitments_errors():
    rng = random.Random(5)

    def drop_size(gi, msg):
        if gi == 0:
            msg.blob_sizes.pop()

    def wrong_size(gi, msg):
        if gi == 2:
            msg.blob_sizes[1] += 1

    def drop_commitment(gi, msg):
        if gi == 2:
            msg.share_commitments.pop()

    def short_commitment(gi, msg):
        if gi == 1:
            msg.share_commitments[0] = msg.share_commitments[0][:31]

    for mutate, err in ((drop_size, "ErrBlobSizeMismatch"), (wrong_size, "ErrBlobSizeMismatch"),
                        (drop_commitment, "ErrInvalidShareCommitments"),
                        (short_commitment, "ErrInvalidShareCommitments")):
        txs, _ = _pfb_block(rng, mutate)
        _, plan = sq.plan_native(txs)
        with pytest.raises(sq.ShareError, match=err):
            sq.expected_commitments(txs, plan)
    # a BlobTx whose inner tx is no PFB
    txs, _ = _pfb_block(rng)
    t, _ = bt.unmarshal_blob_tx(txs[-1])
    txs[-1] = bt.marshal_blob_tx(bt.marshal_sdk_tx("/cosmos.bank.v1beta1.MsgSend", b"\x0a\x01x"), *t.blobs)
    _, plan = sq.plan_native(txs)
    with pytest.raises(bt.BlobTxError, match="ErrNoPFB"):
        sq.expected_commitments(txs, plan)


def test_truncated_plan_is_refused():
    txs, _ = _pfb_block(random.Random(6))
    _, plan = sq.plan_native(txs)
    assert len(sq.plan_blobs(plan)) == 5
    for cut in (plan[:-16], plan[:40], plan[:0]):
        with pytest.raises(ValueError, match="dagpu_square_plan_blobs"):
            sq.plan_blobs(cut.copy())
    # a capacity one too small reports the count
    import ctypes

    from celestia_da import _abi
    n, out = ctypes.c_size_t(0), np.zeros((4, 4), np.uint32)
    p = np.ascontiguousarray(plan)
    assert _abi.lib().dagpu_square_plan_blobs(_abi.addr(p), p.size, _abi.addr(out), 4, ctypes.byref(n)) == _abi.ERR_ARG
    assert n.value == 5 and not out.any()
