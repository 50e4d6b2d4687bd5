"""Protobuf wire format of the two tx envelopes that square construction reads
and writes, and of the MsgPayForBlobs inside a BlobTx's tx (at the end), restated for proto3/gogoproto encoding (fields in number order,
zero values omitted, repeated scalars packed):

  blob.Blob      {bytes namespace_id = 1; bytes data = 2; uint32 share_version = 3;
                  uint32 namespace_version = 4;}         proto/celestia/core/v1/blob/blob.proto
  blob.BlobTx    {bytes tx = 1; repeated Blob blobs = 2; string type_id = 3;}   (type_id "BLOB")
      UnmarshalBlobTx / MarshalBlobTx                     pkg/blob/blob.go:56-90
  tmproto.IndexWrapper {bytes tx = 1; repeated uint32 share_indexes = 2; string type_id = 3;}
      (type_id "INDX"; celestia-core v1.29.0-tm-v0.34.29 proto/tendermint/types/types.proto and
      pkg/consts, not vendored in the reference: restated from the published definitions)

The decoder follows gogoproto's generated Unmarshal: unknown fields are
skipped, a wire type that does not match a known field is an error, and
truncated input is an error.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Tuple

from .shares import NAMESPACE_ID_SIZE, Blob, put_uvarint

PROTO_BLOB_TX_TYPE_ID = "BLOB"
PROTO_INDEX_WRAPPER_TYPE_ID = "INDX"


class ProtoError(ValueError):
    pass


# ---- wire helpers ------------------------------------------------------------------------

def _key(num: int, wt: int) -> bytes:
    return put_uvarint((num << 3) | wt)


def _bytes_field(num: int, v: bytes) -> bytes:
    return _key(num, 2) + put_uvarint(len(v)) + v if v else b""


def _varint_field(num: int, v: int) -> bytes:
    return _key(num, 0) + put_uvarint(v) if v else b""


def _read_varint(buf: bytes, i: int) -> Tuple[int, int]:
    x, s = 0, 0
    while True:
        if i >= len(buf):
            raise ProtoError("unexpected EOF")
        if s >= 64:
            raise ProtoError("integer overflow")
        b = buf[i]
        i += 1
        x |= (b & 0x7F) << s
        if b < 0x80:
            return x & 0xFFFFFFFFFFFFFFFF, i
        s += 7


def _fields(buf: bytes):
    """Yield (field number, wire type, value) with value = int or bytes."""
    i = 0
    while i < len(buf):
        k, i = _read_varint(buf, i)
        num, wt = k >> 3, k & 7
        if num <= 0:
            raise ProtoError(f"illegal tag {num}")
        if wt == 0:
            v, i = _read_varint(buf, i)
        elif wt == 1:
            if i + 8 > len(buf):
                raise ProtoError("unexpected EOF")
            v, i = buf[i:i + 8], i + 8
        elif wt == 2:
            n, i = _read_varint(buf, i)
            if n < 0 or i + n > len(buf):
                raise ProtoError("unexpected EOF")
            v, i = buf[i:i + n], i + n
        elif wt == 5:
            if i + 4 > len(buf):
                raise ProtoError("unexpected EOF")
            v, i = buf[i:i + 4], i + 4
        else:
            raise ProtoError(f"illegal wireType {wt}")
        yield num, wt, v


def _want(wt: int, expect: int, name: str) -> None:
    if wt != expect:
        raise ProtoError(f"wrong wireType = {wt} for field {name}")


# ---- Blob / BlobTx -------------------------------------------------------------------------

def marshal_blob(b: Blob) -> bytes:
    return (_bytes_field(1, b.namespace_id) + _bytes_field(2, b.data)
            + _varint_field(3, b.share_version) + _varint_field(4, b.namespace_version))


def unmarshal_blob(buf: bytes) -> Blob:
    b = Blob(b"", b"", 0, 0)
    for num, wt, v in _fields(buf):
        if num == 1:
            _want(wt, 2, "NamespaceId"); b.namespace_id = bytes(v)
        elif num == 2:
            _want(wt, 2, "Data"); b.data = bytes(v)
        elif num == 3:
            _want(wt, 0, "ShareVersion"); b.share_version = v & 0xFFFFFFFF
        elif num == 4:
            _want(wt, 0, "NamespaceVersion"); b.namespace_version = v & 0xFFFFFFFF
    return b


@dataclass
class BlobTx:
    tx: bytes
    blobs: List[Blob] = field(default_factory=list)
    type_id: str = PROTO_BLOB_TX_TYPE_ID


def marshal_blob_tx(tx: bytes, *blobs: Blob) -> bytes:
    """blob.MarshalBlobTx."""
    out = _bytes_field(1, tx)
    for b in blobs:
        m = marshal_blob(b)
        out += _key(2, 2) + put_uvarint(len(m)) + m
    return out + _bytes_field(3, PROTO_BLOB_TX_TYPE_ID.encode())


def _unmarshal_blob_tx(buf: bytes) -> BlobTx:
    t = BlobTx(b"", [], "")
    for num, wt, v in _fields(buf):
        if num == 1:
            _want(wt, 2, "Tx"); t.tx = bytes(v)
        elif num == 2:
            _want(wt, 2, "Blobs"); t.blobs.append(unmarshal_blob(v))
        elif num == 3:
            _want(wt, 2, "TypeId"); t.type_id = bytes(v).decode("utf-8", "replace")
    return t


def unmarshal_blob_tx(buf: bytes) -> Tuple[BlobTx, bool]:
    """blob.UnmarshalBlobTx: (tx, is_blob_tx)."""
    try:
        t = _unmarshal_blob_tx(buf)
    except ProtoError:
        return BlobTx(b"", [], ""), False
    if t.type_id != PROTO_BLOB_TX_TYPE_ID or not t.blobs:
        return t, False
    if any(len(b.namespace_id) != NAMESPACE_ID_SIZE for b in t.blobs):
        return t, False
    return t, True


# ---- IndexWrapper -------------------------------------------------------------------------

@dataclass
class IndexWrapper:
    tx: bytes
    share_indexes: List[int] = field(default_factory=list)
    type_id: str = PROTO_INDEX_WRAPPER_TYPE_ID

    def marshal(self) -> bytes:
        out = _bytes_field(1, self.tx)
        if self.share_indexes:
            packed = b"".join(put_uvarint(x) for x in self.share_indexes)
            out += _key(2, 2) + put_uvarint(len(packed)) + packed
        return out + _bytes_field(3, self.type_id.encode())

    def size(self) -> int:
        return len(self.marshal())


def unmarshal_index_wrapper(buf: bytes) -> Tuple[Optional[IndexWrapper], bool]:
    """types.UnmarshalIndexWrapper: (wrapper, is_index_wrapper)."""
    iw = IndexWrapper(b"", [], "")
    try:
        for num, wt, v in _fields(buf):
            if num == 1:
                _want(wt, 2, "Tx"); iw.tx = bytes(v)
            elif num == 2:
                if wt == 0:
                    iw.share_indexes.append(v & 0xFFFFFFFF)
                elif wt == 2:
                    j = 0
                    while j < len(v):
                        x, j = _read_varint(v, j)
                        iw.share_indexes.append(x & 0xFFFFFFFF)
                else:
                    raise ProtoError(f"wrong wireType = {wt} for field ShareIndexes")
            elif num == 3:
                _want(wt, 2, "TypeId"); iw.type_id = bytes(v).decode("utf-8", "replace")
    except ProtoError:
        return None, False
    if iw.type_id != PROTO_INDEX_WRAPPER_TYPE_ID:
        return None, False
    return iw, True


# ---- MsgPayForBlobs inside an sdk.Tx ---------------------------------------------------------
# celestia.blob.v1.MsgPayForBlobs {string signer = 1; repeated bytes namespaces = 2;
#   repeated uint32 blob_sizes = 3; repeated bytes share_commitments = 4;
#   repeated uint32 share_versions = 8;}                    proto/celestia/blob/v1/tx.proto
# cosmos.tx.v1beta1.Tx {TxBody body = 1; AuthInfo auth_info = 2; repeated bytes signatures = 3;}
#   TxBody {repeated google.protobuf.Any messages = 1; ...}  Any {string type_url = 1; bytes value = 2;}
# ValidateBlobTx (x/blob/types/blob_tx.go:36-100) decodes the BlobTx's inner tx, wants exactly one
# message, a MsgPayForBlobs, and compares its sizes and share commitments with the blobs.

URL_MSG_PAY_FOR_BLOBS = "/celestia.blob.v1.MsgPayForBlobs"


class BlobTxError(ValueError):
    """A ValidateBlobTx failure; `name` is the reference's error name."""

    def __init__(self, name: str, msg: str):
        super().__init__(f"{name}: {msg}")
        self.name = name


@dataclass
class MsgPayForBlobs:
    signer: str = ""
    namespaces: List[bytes] = field(default_factory=list)
    blob_sizes: List[int] = field(default_factory=list)
    share_commitments: List[bytes] = field(default_factory=list)
    share_versions: List[int] = field(default_factory=list)

    def marshal(self, packed: bool = True) -> bytes:
        """gogoproto's encoding (repeated uint32 packed); packed=False writes the
        one-varint-per-element form that every proto3 decoder must accept too."""
        def repeated_u32(num: int, vals) -> bytes:
            if not vals:
                return b""
            if not packed:
                return b"".join(_key(num, 0) + put_uvarint(v) for v in vals)
            body = b"".join(put_uvarint(v) for v in vals)
            return _key(num, 2) + put_uvarint(len(body)) + body

        out = _bytes_field(1, self.signer.encode())
        for ns in self.namespaces:  # repeated bytes: empty elements are written too
            out += _key(2, 2) + put_uvarint(len(ns)) + ns
        out += repeated_u32(3, self.blob_sizes)
        for c in self.share_commitments:
            out += _key(4, 2) + put_uvarint(len(c)) + c
        return out + repeated_u32(8, self.share_versions)


def _repeated_u32(wt: int, v, into: List[int], name: str) -> None:
    if wt == 0:
        into.append(v & 0xFFFFFFFF)
    elif wt == 2:
        j = 0
        while j < len(v):
            x, j = _read_varint(v, j)
            into.append(x & 0xFFFFFFFF)
    else:
        raise ProtoError(f"wrong wireType = {wt} for field {name}")


def unmarshal_msg_pay_for_blobs(buf: bytes) -> MsgPayForBlobs:
    m = MsgPayForBlobs()
    for num, wt, v in _fields(buf):
        if num == 1:
            _want(wt, 2, "Signer"); m.signer = bytes(v).decode("utf-8", "replace")
        elif num == 2:
            _want(wt, 2, "Namespaces"); m.namespaces.append(bytes(v))
        elif num == 3:
            _repeated_u32(wt, v, m.blob_sizes, "BlobSizes")
        elif num == 4:
            _want(wt, 2, "ShareCommitments"); m.share_commitments.append(bytes(v))
        elif num == 8:
            _repeated_u32(wt, v, m.share_versions, "ShareVersions")
    return m


def marshal_sdk_tx(msg_type_url: str, msg_value: bytes, auth_info: bytes = b"", signatures=(),
                   extra_msgs=()) -> bytes:
    """A decodable cosmos Tx around one message (and extra_msgs: further
    (type_url, value) pairs): body 1 {messages 1: Any {type_url 1, value 2}},
    auth_info 2, signatures 3."""
    body = b""
    for url, val in ((msg_type_url, msg_value),) + tuple(extra_msgs):
        any_ = _bytes_field(1, url.encode()) + _bytes_field(2, val)
        body += _key(1, 2) + put_uvarint(len(any_)) + any_
    out = _key(1, 2) + put_uvarint(len(body)) + body + _bytes_field(2, auth_info)
    for sig in signatures:
        out += _key(3, 2) + put_uvarint(len(sig)) + sig
    return out


def sdk_tx_messages(tx: bytes) -> List[Tuple[str, bytes]]:
    """(type_url, value) of every message of a cosmos Tx."""
    msgs = []
    for num, wt, v in _fields(tx):
        if num != 1:
            continue
        _want(wt, 2, "Body")
        for bnum, bwt, bv in _fields(v):
            if bnum != 1:
                continue
            _want(bwt, 2, "Messages")
            url, val = "", b""
            for anum, awt, av in _fields(bv):
                if anum == 1:
                    _want(awt, 2, "TypeUrl"); url = bytes(av).decode("utf-8", "replace")
                elif anum == 2:
                    _want(awt, 2, "Value"); val = bytes(av)
            msgs.append((url, val))
    return msgs


def pfb_of_tx(tx: bytes) -> MsgPayForBlobs:
    """The MsgPayForBlobs of a BlobTx's inner tx (blob_tx.go:41-52): exactly
    one message (ErrMultipleMsgsInBlobTx) of that type (ErrNoPFB)."""
    msgs = sdk_tx_messages(tx)
    if len(msgs) != 1:
        raise BlobTxError("ErrMultipleMsgsInBlobTx", f"{len(msgs)} sdk.Msgs found in BlobTx")
    url, val = msgs[0]
    if url != URL_MSG_PAY_FOR_BLOBS:
        raise BlobTxError("ErrNoPFB", f"no MsgPayForBlobs found in blob transaction (message {url!r})")
    return unmarshal_msg_pay_for_blobs(val)


def blob_data_offsets(raw_blob_tx: bytes) -> List[Tuple[int, int]]:
    """(offset, length) of each blob's `data` field inside the raw BlobTx
    bytes, in blob order; a blob without data gets (offset of its end, 0)."""
    out = []
    i = 0
    while i < len(raw_blob_tx):
        k, i = _read_varint(raw_blob_tx, i)
        num, wt = k >> 3, k & 7
        if wt == 0:
            _, i = _read_varint(raw_blob_tx, i)
            continue
        if wt in (1, 5):
            i += 8 if wt == 1 else 4
            continue
        if wt != 2:
            raise ProtoError(f"illegal wireType {wt}")
        n, i = _read_varint(raw_blob_tx, i)
        if i + n > len(raw_blob_tx):
            raise ProtoError("unexpected EOF")
        if num == 2:  # one Blob: find its data field (the last one wins, as in Unmarshal)
            j, end, found = i, i + n, (i + n, 0)
            while j < end:
                bk, j = _read_varint(raw_blob_tx, j)
                bnum, bwt = bk >> 3, bk & 7
                if bwt == 0:
                    _, j = _read_varint(raw_blob_tx, j)
                elif bwt == 2:
                    bn, j = _read_varint(raw_blob_tx, j)
                    if j + bn > end:
                        raise ProtoError("unexpected EOF")
                    if bnum == 2:
                        found = (j, bn)
                    j += bn
                elif bwt in (1, 5):
                    j += 8 if bwt == 1 else 4
                else:
                    raise ProtoError(f"illegal wireType {bwt}")
            out.append(found)
        i += n
    return out
