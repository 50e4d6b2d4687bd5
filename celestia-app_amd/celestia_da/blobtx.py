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

    def __init__(self, name: str, msg: str, kind: str = "", index: int = 0):
        super().__init__(f"{name}: {msg}")
        self.name = name
        # validate_blob_tx: the kind of KIND_NAMES and the index the native word carries
        self.kind, self.index = kind, index


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


# ---- ValidateBlobTx, the stateless rules (x/blob/types/blob_tx.go:36-103) -----------------------
# The readable mirror of csrc/blobtx_check.hpp, written independently of it: the same rules in
# the same order over the decoded objects.  The native per-tx word is kind | index << 8
# (dagpu_blob_tx_check, include/dagpu.h DAGPU_BLOBTX_*).

KIND_NAMES = (
    "OK", "DECODE", "MULTIPLE_MSGS", "NO_PFB", "PFB_DECODE", "NO_NAMESPACES", "NO_SHARE_VERSIONS",
    "NO_BLOB_SIZES", "NO_SHARE_COMMITMENTS", "MISMATCHED_COUNTS", "INVALID_NAMESPACE", "RESERVED_NAMESPACE",
    "INVALID_NAMESPACE_VERSION", "UNSUPPORTED_SHARE_VERSION", "BAD_SIGNER", "BAD_COMMITMENT_LENGTH",
    "BLOB_NAMESPACE_VERSION_TOO_LARGE", "BLOB_INVALID_NAMESPACE", "BLOB_RESERVED_NAMESPACE",
    "BLOB_INVALID_NAMESPACE_VERSION", "ZERO_BLOB_SIZE", "BLOB_UNSUPPORTED_SHARE_VERSION", "SIZE_MISMATCH",
    "NAMESPACE_MISMATCH", "NON_BLOB_TX_HAS_PFB")

# kind -> the reference's error (x/blob/types/errors.go), or what stands in for one it takes from
# elsewhere: the TxDecoder's and the unpacker's errors, bech32's, fmt.Errorf at payforblob.go:218
# and namespace.New's
_ERR_OF = {
    "DECODE": "ErrTxDecode", "MULTIPLE_MSGS": "ErrMultipleMsgsInBlobTx", "NO_PFB": "ErrNoPFB",
    "PFB_DECODE": "ErrTxDecode", "NO_NAMESPACES": "ErrNoNamespaces", "NO_SHARE_VERSIONS": "ErrNoShareVersions",
    "NO_BLOB_SIZES": "ErrNoBlobSizes", "NO_SHARE_COMMITMENTS": "ErrNoShareCommitments",
    "MISMATCHED_COUNTS": "ErrMismatchedNumberOfPFBComponent", "INVALID_NAMESPACE": "ErrInvalidNamespace",
    "RESERVED_NAMESPACE": "ErrReservedNamespace", "INVALID_NAMESPACE_VERSION": "ErrInvalidNamespaceVersion",
    "UNSUPPORTED_SHARE_VERSION": "ErrUnsupportedShareVersion", "BAD_SIGNER": "ErrInvalidAddress",
    "BAD_COMMITMENT_LENGTH": "ErrInvalidShareCommitment",
    "BLOB_NAMESPACE_VERSION_TOO_LARGE": "namespace version is too large",
    "BLOB_INVALID_NAMESPACE": "unsupported namespace", "BLOB_RESERVED_NAMESPACE": "ErrReservedNamespace",
    "BLOB_INVALID_NAMESPACE_VERSION": "ErrInvalidNamespaceVersion", "ZERO_BLOB_SIZE": "ErrZeroBlobSize",
    "BLOB_UNSUPPORTED_SHARE_VERSION": "ErrUnsupportedShareVersion", "SIZE_MISMATCH": "ErrBlobSizeMismatch",
    "NAMESPACE_MISMATCH": "ErrNamespaceMismatch", "NON_BLOB_TX_HAS_PFB": "tx has PFB but is not a blob tx",
}


def error_name(kind: int) -> str:
    """The reference's error for a kind of KIND_NAMES (see _ERR_OF)."""
    return _ERR_OF[KIND_NAMES[kind]]


BECH32_CHARSET = "qpzry9x8gf2tvdw0s3jn54khce6mua7l"
ACCOUNT_HRP = "celestia"


def _fail(kind: str, index: int = 0, msg: str = ""):
    return BlobTxError(_ERR_OF[kind], msg or kind, kind=kind, index=min(index, (1 << 24) - 1))


def _bech32_polymod(values) -> int:
    chk = 1
    for v in values:
        top = chk >> 25
        chk = ((chk & 0x1FFFFFF) << 5) ^ v
        for i, g in enumerate((0x3B6A57B2, 0x26508E6D, 0x1EA119FA, 0x3D4233DD, 0x2A1462B3)):
            if (top >> i) & 1:
                chk ^= g
    return chk


def bech32_decode(addr: str) -> Tuple[str, bytes]:
    """BIP-173 bech32 as sdk.AccAddressFromBech32 uses it: (hrp, the data
    regrouped from 5 to 8 bits without padding).  Raises ValueError.  The SDK
    is not vendored in the reference: recalled, parity unpinned beyond the
    addresses the reference's own files contain."""
    if any(ord(c) < 33 or ord(c) > 126 for c in addr):
        raise ValueError("bech32: character out of range")
    if addr.lower() != addr and addr.upper() != addr:
        raise ValueError("bech32: mixed case")
    addr = addr.lower()
    sep = addr.rfind("1")
    if sep < 1 or len(addr) - sep - 1 < 6:
        raise ValueError("bech32: separator")
    hrp, data = addr[:sep], []
    for c in addr[sep + 1:]:
        v = BECH32_CHARSET.find(c)
        if v < 0:
            raise ValueError(f"bech32: invalid character {c!r}")
        data.append(v)
    if _bech32_polymod([ord(c) >> 5 for c in hrp] + [0] + [ord(c) & 31 for c in hrp] + data) != 1:
        raise ValueError("bech32: checksum")
    acc = bits = 0
    out = bytearray()
    for v in data[:-6]:
        acc = (acc << 5) | v
        bits += 5
        if bits >= 8:
            bits -= 8
            out.append((acc >> bits) & 0xFF)
    if bits >= 5 or acc & ((1 << bits) - 1):
        raise ValueError("bech32: padding")
    return hrp, bytes(out)


def acc_address_from_bech32(signer: str) -> bytes:
    """sdk.AccAddressFromBech32 with the prefix "celestia" (see bech32_decode)."""
    if not signer.strip(" "):
        raise ValueError("empty address string is not allowed")
    hrp, raw = bech32_decode(signer)
    if hrp != ACCOUNT_HRP:
        raise ValueError(f"invalid Bech32 prefix; expected {ACCOUNT_HRP}, got {hrp}")
    if not 1 <= len(raw) <= 255:
        raise ValueError("address length")
    return raw


def _namespace_rule(ns: bytes) -> str:
    """namespace.From / New, then ValidateBlobNamespace (payforblob.go:183-193):
    "" or INVALID_NAMESPACE / RESERVED_NAMESPACE / INVALID_NAMESPACE_VERSION."""
    if len(ns) != 29 or ns[0] not in (0, 255) or (ns[0] == 0 and any(ns[1:19])):
        return "INVALID_NAMESPACE"
    if ns <= bytes(28) + b"\xff" or ns >= b"\xff" * 28 + b"\x00":
        return "RESERVED_NAMESPACE"
    return "" if ns[0] == 0 else "INVALID_NAMESPACE_VERSION"


def validate_blob_tx(raw: bytes) -> None:
    """ValidateBlobTx short of the comparison of the commitments themselves
    (blob_tx.go:92-100; check_commitments makes it on the device): raises
    BlobTxError for the first rule `raw`, a BlobTx, breaks, with the
    reference's error name and .kind / .index as the native word carries them.
    ValueError when raw is no BlobTx."""
    t, ok = unmarshal_blob_tx(bytes(raw))
    if not ok:
        raise ValueError("not a BlobTx")
    try:
        msgs = sdk_tx_messages(t.tx)
    except ProtoError as e:
        raise _fail("DECODE", 0, str(e))
    if len(msgs) != 1:
        raise _fail("MULTIPLE_MSGS", len(msgs), f"{len(msgs)} sdk.Msgs found in BlobTx")
    if msgs[0][0] != URL_MSG_PAY_FOR_BLOBS:
        raise _fail("NO_PFB")
    try:
        pfb = unmarshal_msg_pay_for_blobs(msgs[0][1])
    except ProtoError as e:
        raise _fail("PFB_DECODE", 0, str(e))
    # MsgPayForBlobs.ValidateBasic (payforblob.go:95-148)
    if not pfb.namespaces:
        raise _fail("NO_NAMESPACES")
    if not pfb.share_versions:
        raise _fail("NO_SHARE_VERSIONS")
    if not pfb.blob_sizes:
        raise _fail("NO_BLOB_SIZES")
    if not pfb.share_commitments:
        raise _fail("NO_SHARE_COMMITMENTS")
    if not len(pfb.namespaces) == len(pfb.share_versions) == len(pfb.blob_sizes) == len(pfb.share_commitments):
        raise _fail("MISMATCHED_COUNTS")
    for i, ns in enumerate(pfb.namespaces):
        rule = _namespace_rule(ns)
        if rule:
            raise _fail(rule, i)
    for i, v in enumerate(pfb.share_versions):
        if v != 0:
            raise _fail("UNSUPPORTED_SHARE_VERSION", i)
    try:
        acc_address_from_bech32(pfb.signer)
    except ValueError as e:
        raise _fail("BAD_SIGNER", 0, str(e))
    for i, c in enumerate(pfb.share_commitments):
        if len(c) != 32:
            raise _fail("BAD_COMMITMENT_LENGTH", i)
    # ValidateBlobs (payforblob.go:211-239)
    for i, b in enumerate(t.blobs):
        if b.namespace_version > 255:
            raise _fail("BLOB_NAMESPACE_VERSION_TOO_LARGE", i)
        rule = _namespace_rule(bytes([b.namespace_version]) + b.namespace_id)
        if rule:
            raise _fail("BLOB_" + rule, i)
        if len(b.data) == 0:
            raise _fail("ZERO_BLOB_SIZE", i)
        if b.share_version & 0xFF != 0:
            raise _fail("BLOB_UNSUPPORTED_SHARE_VERSION", i)
    sizes = [len(b.data) for b in t.blobs]
    if len(sizes) != len(pfb.blob_sizes):
        raise _fail("SIZE_MISMATCH", min(len(sizes), len(pfb.blob_sizes)))
    for i, (got, declared) in enumerate(zip(sizes, pfb.blob_sizes)):
        if got != declared:
            raise _fail("SIZE_MISMATCH", i, f"actual {sizes} declared {pfb.blob_sizes}")
    for i, ns in enumerate(pfb.namespaces):
        if bytes([t.blobs[i].namespace_version]) + t.blobs[i].namespace_id != ns:
            raise _fail("NAMESPACE_MISMATCH", i)


def check_tx(raw: bytes) -> Tuple[int, int]:
    """(kind, index) of any tx as ProcessProposal's loop sees it
    (process_proposal.go:60-77, :120), from the mirror: validate_blob_tx for a
    BlobTx; for any other tx NON_BLOB_TX_HAS_PFB with the first such message
    when it decodes and holds a MsgPayForBlobs, else (0, 0)."""
    raw = bytes(raw)
    if unmarshal_blob_tx(raw)[1]:
        try:
            validate_blob_tx(raw)
        except BlobTxError as e:
            return KIND_NAMES.index(e.kind), e.index
        return 0, 0
    try:
        urls = [u for u, _ in sdk_tx_messages(raw)]
    except ProtoError:
        return 0, 0
    if URL_MSG_PAY_FOR_BLOBS in urls:
        return KIND_NAMES.index("NON_BLOB_TX_HAS_PFB"), min(urls.index(URL_MSG_PAY_FOR_BLOBS), (1 << 24) - 1)
    return 0, 0


def check_native(raw: bytes) -> Tuple[int, int]:
    """(kind, index) of one tx through dagpu_blob_tx_check (csrc/blobtx_check.hpp)."""
    import numpy as np

    from . import _abi
    buf = np.frombuffer(bytes(raw), np.uint8)
    word = _abi.lib().dagpu_blob_tx_check(_abi.addr(buf) if buf.size else None, buf.size)
    return word & 0xFF, word >> 8


# ---- tx signatures: SIGN_MODE_DIRECT over secp256k1 (cosmos-sdk v0.46 x/auth/ante/sigverify.go) --------
# The readable mirror of csrc/tx_sig.hpp, written independently of it (the curve is secp256k1.py).
#   TxRaw      {bytes body_bytes = 1; bytes auth_info_bytes = 2; repeated bytes signatures = 3;}
#   AuthInfo   {repeated SignerInfo signer_infos = 1; Fee fee = 2;}
#   SignerInfo {Any public_key = 1; ModeInfo mode_info = 2; uint64 sequence = 3;}
#   ModeInfo   {oneof sum {Single single = 1 {SignMode mode = 1;}; Multi multi = 2;}}
#   SignDoc    {bytes body_bytes = 1; bytes auth_info_bytes = 2; string chain_id = 3; uint64 account_number = 4;}
# A word is (kind, index), kind a key of _abi.SIG_KIND_NAMES (include/dagpu.h DAGPU_SIG_*).

URL_SECP256K1_PUBKEY = "/cosmos.crypto.secp256k1.PubKey"
SIGN_MODE_DIRECT = 1
_SIG_CAP = (1 << 24) - 1


def _wrap(num: int, v: bytes) -> bytes:
    """A length-delimited field that is written even when empty."""
    return _key(num, 2) + put_uvarint(len(v)) + v


def marshal_signer_info(pubkey: Optional[bytes], sequence: int, mode: int = SIGN_MODE_DIRECT,
                        type_url: str = URL_SECP256K1_PUBKEY, multi: bool = False) -> bytes:
    out = b""
    if pubkey is not None:
        out += _wrap(1, _bytes_field(1, type_url.encode()) + _bytes_field(2, _bytes_field(1, bytes(pubkey))))
    mode_info = _wrap(2, b"") if multi else _wrap(1, _varint_field(1, mode))
    return out + _wrap(2, mode_info) + _varint_field(3, sequence)


def marshal_auth_info(pubkey: Optional[bytes], sequence: int, mode: int = SIGN_MODE_DIRECT,
                      type_url: str = URL_SECP256K1_PUBKEY, multi: bool = False, signers: int = 1,
                      fee: bytes = b"") -> bytes:
    """AuthInfo with `signers` copies of one SignerInfo (pubkey None: no
    public_key; multi: ModeInfo.Multi) and an opaque fee."""
    si = marshal_signer_info(pubkey, sequence, mode, type_url, multi)
    return b"".join(_wrap(1, si) for _ in range(signers)) + _bytes_field(2, fee)


def _inner_tx(raw: bytes) -> bytes:
    t, is_blob = unmarshal_blob_tx(bytes(raw))
    return t.tx if is_blob else bytes(raw)


def _tx_raw(inner: bytes):
    body, auth, sigs = b"", b"", []
    for num, wt, v in _fields(inner):
        if num == 1:
            _want(wt, 2, "BodyBytes"); body = bytes(v)
        elif num == 2:
            _want(wt, 2, "AuthInfoBytes"); auth = bytes(v)
        elif num == 3:
            _want(wt, 2, "Signatures"); sigs.append(bytes(v))
    return body, auth, sigs


def sign_doc_bytes(tx: bytes, chain_id, account_number: int) -> bytes:
    """DirectSignBytes of a tx (a BlobTx: of its inner tx): the SignDoc over
    the exact body_bytes and auth_info_bytes ranges; empty and zero fields
    are omitted."""
    body, auth, _ = _tx_raw(_inner_tx(tx))
    chain = chain_id.encode() if isinstance(chain_id, str) else bytes(chain_id)
    return _bytes_field(1, body) + _bytes_field(2, auth) + _bytes_field(3, chain) + _varint_field(4, account_number)


def _walk_signer(raw: bytes):
    """(kind, index, key or None, sequence, signature) as the walk alone
    classifies a tx: no table, no curve arithmetic."""
    inner = _inner_tx(raw)
    try:
        _, auth, sigs = _tx_raw(inner)
        sdk_tx_messages(inner)
        infos = []
        for num, wt, v in _fields(auth):
            if num == 1:
                _want(wt, 2, "SignerInfos"); infos.append(bytes(v))
        if len(infos) != 1 or len(sigs) != 1:
            return 2, min(len(infos), _SIG_CAP), None, 0, b""
        any_, mode_info, sequence = None, b"", 0
        for num, wt, v in _fields(infos[0]):
            if num == 1:
                _want(wt, 2, "PublicKey"); any_ = bytes(v)
            elif num == 2:
                _want(wt, 2, "ModeInfo"); mode_info = bytes(v)
            elif num == 3:
                _want(wt, 0, "Sequence"); sequence = v
        which, single, mode = 0, b"", 0
        for num, wt, v in _fields(mode_info):
            if num in (1, 2):
                _want(wt, 2, "Sum"); which = num
                if num == 1:
                    single = bytes(v)
        if which == 1:
            for num, wt, v in _fields(single):
                if num == 1:
                    _want(wt, 0, "Mode"); mode = v & 0xFFFFFFFF
        url, value = b"", b""
        if any_ is not None:
            for num, wt, v in _fields(any_):
                if num == 1:
                    _want(wt, 2, "TypeUrl"); url = bytes(v)
                elif num == 2:
                    _want(wt, 2, "Value"); value = bytes(v)
        if which != 1:
            return 3, 0, None, sequence, sigs[0]
        if mode != SIGN_MODE_DIRECT:
            return 3, min(mode, _SIG_CAP), None, sequence, sigs[0]
        key = None
        if any_ is not None:
            if url != URL_SECP256K1_PUBKEY.encode():
                return 4, 0, None, sequence, sigs[0]
            key = b""
            for num, wt, v in _fields(value):
                if num == 1:
                    _want(wt, 2, "Key"); key = bytes(v)
    except ProtoError:
        return 1, 0, None, 0, b""
    if key is None:
        return 5, 0, None, sequence, sigs[0]
    if len(key) != 33:
        return 16, 0, key, sequence, sigs[0]
    if len(sigs[0]) != 64:
        return 17, min(len(sigs[0]), _SIG_CAP), key, sequence, sigs[0]
    return 0, 0, key, sequence, sigs[0]


def signer_of_tx(tx: bytes) -> Tuple[bytes, int, int]:
    """(pubkey, kind, sequence) as dagpu_tx_signers_* records them: the 33-byte
    key the tx carries (33 zeros when it carries none of that length), the
    kind the walk alone gives, the sequence it declares."""
    kind, _, key, sequence, _ = _walk_signer(bytes(tx))
    return (key if key is not None and len(key) == 33 else bytes(33)), kind, sequence


def check_signature(tx: bytes, chain_id, account_number: int, pubkey: Optional[bytes] = None) -> Tuple[int, int]:
    """(kind, index) of one tx as dagpu_tx_sig_verify_* gives it.  pubkey: the
    account's stored key (33 bytes), used instead of the tx's own when given."""
    from . import _abi, secp256k1 as ec
    tx = bytes(tx)
    kind, index, key, _, sig = _walk_signer(tx)
    if 1 <= kind <= 4:
        return kind, index
    if pubkey is not None:
        key = bytes(pubkey)
    elif kind in (5, 16):
        return kind, index
    if ec.decompress(key) is None:
        return 16, 0
    if len(sig) != 64:
        return 17, min(len(sig), _SIG_CAP)
    return _abi.SIG_KINDS[ec.verify(key, sign_doc_bytes(tx, chain_id, account_number), sig)], 0
