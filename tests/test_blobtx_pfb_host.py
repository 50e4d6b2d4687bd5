"""MsgPayForBlobs inside a cosmos Tx inside a BlobTx (celestia_da/blobtx.py):
the message's wire format with packed and unpacked repeated uint32, the
one-message rule of ValidateBlobTx with the reference's error names, and the
offsets of every blob's data inside the raw BlobTx bytes."""
import random

import pytest

from celestia_da import blobtx as bt
from celestia_da import shares as sh

NS = [sh.new_namespace_v0(bytes([i]) * 10) for i in range(1, 6)]


def _msg(n, rng):
    return bt.MsgPayForBlobs(signer="celestia1" + "q" * 38, namespaces=[NS[i % 5] for i in range(n)],
                             blob_sizes=[rng.choice([1, 127, 128, 16384, 70000, 2**32 - 1]) for _ in range(n)],
                             share_commitments=[rng.randbytes(32) for _ in range(n)], share_versions=[0] * n)


def test_msg_pay_for_blobs_round_trip():
    rng = random.Random(1)
    for n in (0, 1, 2, 5):
        m = _msg(n, rng)
        packed, unpacked = m.marshal(), m.marshal(packed=False)
        assert bt.unmarshal_msg_pay_for_blobs(packed) == m
        assert bt.unmarshal_msg_pay_for_blobs(unpacked) == m
        assert (packed == unpacked) == (n == 0)
    # share_versions of zero are written in the packed form (one byte each), not dropped
    m = _msg(2, rng)
    assert m.marshal().endswith(b"\x42\x02\x00\x00")
    # a mix of both forms in one message concatenates
    one = bt.MsgPayForBlobs(blob_sizes=[7]).marshal(packed=False) + bt.MsgPayForBlobs(blob_sizes=[8, 300]).marshal()
    assert bt.unmarshal_msg_pay_for_blobs(one).blob_sizes == [7, 8, 300]
    # unknown fields are skipped, a wrong wire type for a known field is an error
    assert bt.unmarshal_msg_pay_for_blobs(b"\x28\x05" + m.marshal()) == m
    with pytest.raises(bt.ProtoError):
        bt.unmarshal_msg_pay_for_blobs(b"\x1d\x00\x00\x00\x00")  # field 3 as fixed32
    with pytest.raises(bt.ProtoError):
        bt.unmarshal_msg_pay_for_blobs(m.marshal()[:-1] + b"\x80")


def test_pfb_of_tx():
    rng = random.Random(2)
    m = _msg(3, rng)
    tx = bt.marshal_sdk_tx(bt.URL_MSG_PAY_FOR_BLOBS, m.marshal(), auth_info=b"\x12\x04fees", signatures=[b"s" * 64])
    assert bt.sdk_tx_messages(tx) == [(bt.URL_MSG_PAY_FOR_BLOBS, m.marshal())]
    assert bt.pfb_of_tx(tx) == m
    two = bt.marshal_sdk_tx(bt.URL_MSG_PAY_FOR_BLOBS, m.marshal(),
                            extra_msgs=[(bt.URL_MSG_PAY_FOR_BLOBS, m.marshal())])
    with pytest.raises(bt.BlobTxError, match="ErrMultipleMsgsInBlobTx") as e:
        bt.pfb_of_tx(two)
    assert e.value.name == "ErrMultipleMsgsInBlobTx"
    with pytest.raises(bt.BlobTxError, match="ErrMultipleMsgsInBlobTx"):
        bt.pfb_of_tx(b"")  # no message at all
    send = bt.marshal_sdk_tx("/cosmos.bank.v1beta1.MsgSend", b"\x0a\x03abc")
    with pytest.raises(bt.BlobTxError, match="ErrNoPFB") as e:
        bt.pfb_of_tx(send)
    assert e.value.name == "ErrNoPFB"


@pytest.mark.parametrize("sizes", [(1,), (16384, 1), (1, 127, 128, 20000, 3)])
def test_blob_data_offsets(sizes):
    """1, 2 and 5 blobs; data of 1 byte (the smallest), 127 / 128 (the length
    varint grows to two bytes) and >= 16 KiB (three bytes)."""
    rng = random.Random(len(sizes))
    blobs = [sh.Blob.new(NS[i], rng.randbytes(n)) for i, n in enumerate(sizes)]
    m = bt.MsgPayForBlobs(signer="s", namespaces=[b.namespace() for b in blobs], blob_sizes=list(sizes),
                          share_commitments=[rng.randbytes(32) for _ in blobs], share_versions=[0] * len(blobs))
    raw = bt.marshal_blob_tx(bt.marshal_sdk_tx(bt.URL_MSG_PAY_FOR_BLOBS, m.marshal()), *blobs)
    offs = bt.blob_data_offsets(raw)
    assert len(offs) == len(blobs)
    for (off, ln), b in zip(offs, blobs):
        assert ln == len(b.data) and raw[off:off + ln] == b.data
    assert [o for o, _ in offs] == sorted(o for o, _ in offs)
    t, ok = bt.unmarshal_blob_tx(raw)
    assert ok and bt.pfb_of_tx(t.tx) == m and [b.data for b in t.blobs] == [b.data for b in blobs]
    with pytest.raises(bt.ProtoError):
        bt.blob_data_offsets(raw[:offs[-1][0] + 1] if sizes[-1] > 1 else raw[:offs[-1][0]])
