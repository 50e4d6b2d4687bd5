"""Txs, blocks and helpers shared by test_blobtx_validate_host.py and
test_gpu_blobtx_validate_device.py: valid BlobTxs around a real MsgPayForBlobs
(marshal_sdk_tx(URL_MSG_PAY_FOR_BLOBS, MsgPayForBlobs(...).marshal())), one tx
per kind of blobtx.KIND_NAMES, and dagpu_blob_tx_validate_host as a function."""
import random

import numpy as np

import pyref
from celestia_da import _abi, blobtx as bt, shares as sh, square as sq

# the addresses the reference's own files contain: test/util/testfactory/common.go:20,
# scripts/README.md:26, specs/src/specs/public_key_cryptography.md:31
ADDRS = ("celestia1g39egf59z8tud3lcyjg5a83m20df4kccx32qkp",
         "celestia1grvklux2yjsln7ztk6slv538396qatckqhs86z",
         "celestia1kj39jkzqlr073t42am9d8pd40tgudc3e2kj9yf")
NS = [sh.new_namespace_v0(bytes([i]) * 10) for i in range(1, 9)]
URL_SEND = "/cosmos.bank.v1beta1.MsgSend"
K = {name: i for i, name in enumerate(bt.KIND_NAMES)}

_commitments = {}


def commitment(b: sh.Blob) -> bytes:
    key = (b.namespace(), b.data)
    if key not in _commitments:
        _commitments[key] = pyref.create_commitment(b.namespace(), b.data)
    return _commitments[key]


def pfb_of(blobs, signer=ADDRS[0]) -> bt.MsgPayForBlobs:
    return bt.MsgPayForBlobs(signer=signer, namespaces=[b.namespace() for b in blobs],
                             blob_sizes=[len(b.data) for b in blobs],
                             share_commitments=[commitment(b) for b in blobs], share_versions=[0] * len(blobs))


def blob_tx(blobs, pfb=None, inner=None, packed=True) -> bytes:
    """A BlobTx of `blobs` around `inner`, by default the sdk tx of `pfb`, by
    default the valid MsgPayForBlobs of the blobs."""
    if inner is None:
        pfb = pfb_of(blobs) if pfb is None else pfb
        inner = bt.marshal_sdk_tx(bt.URL_MSG_PAY_FOR_BLOBS, pfb.marshal(packed=packed), auth_info=b"\x12\x04fees",
                                  signatures=[b"s" * 64])
    return bt.marshal_blob_tx(inner, *blobs)


def blobs_of(rng, n, sizes=(1, 100, 477, 478, 479, 1200), namespaces=NS):
    return [sh.Blob.new(rng.choice(namespaces), rng.randbytes(rng.choice(sizes))) for _ in range(n)]


def valid_tx(rng, n=1, signer=None, **kw) -> bytes:
    blobs = blobs_of(rng, n, **kw)
    return blob_tx(blobs, pfb_of(blobs, signer or rng.choice(ADDRS)))


def normal_tx(rng) -> bytes:
    return bt.marshal_sdk_tx(URL_SEND, rng.randbytes(rng.randrange(1, 200)), signatures=[rng.randbytes(64)])


def kind_cases():
    """{kind name: (raw tx, index)}: one tx per kind, each with exactly that
    first fault."""
    rng = random.Random(7)
    two = [sh.Blob.new(NS[0], rng.randbytes(300)), sh.Blob.new(NS[1], rng.randbytes(20))]

    def with_pfb(blobs=two, **over):
        p = pfb_of(blobs)
        for name, v in over.items():
            setattr(p, name, v)
        return blob_tx(blobs, p)

    def with_blob(**over):
        b = sh.Blob.new(NS[1], rng.randbytes(20))
        for name, v in over.items():
            setattr(b, name, v)
        good = sh.Blob.new(NS[0], rng.randbytes(300))
        p = pfb_of([good, sh.Blob.new(NS[1], rng.randbytes(max(1, len(b.data))))])
        p.blob_sizes[1] = len(b.data)
        return blob_tx([good, b], p)

    pfb = pfb_of(two).marshal()
    replaced = lambda seq, i, v: seq[:i] + [v] + seq[i + 1:]
    p = pfb_of(two)
    cases = {
        "OK": (blob_tx(two), 0),
        "DECODE": (blob_tx(two, inner=b"\x0a\x05abc"), 0),
        "MULTIPLE_MSGS": (blob_tx(two, inner=bt.marshal_sdk_tx(bt.URL_MSG_PAY_FOR_BLOBS, pfb,
                                                               extra_msgs=[(bt.URL_MSG_PAY_FOR_BLOBS, pfb)])), 2),
        "NO_PFB": (blob_tx(two, inner=bt.marshal_sdk_tx(URL_SEND, pfb)), 0),
        "PFB_DECODE": (blob_tx(two, inner=bt.marshal_sdk_tx(bt.URL_MSG_PAY_FOR_BLOBS, b"\x1d\x00\x00\x00\x00")), 0),
        "NO_NAMESPACES": (with_pfb(namespaces=[]), 0),
        "NO_SHARE_VERSIONS": (with_pfb(share_versions=[]), 0),
        "NO_BLOB_SIZES": (with_pfb(blob_sizes=[]), 0),
        "NO_SHARE_COMMITMENTS": (with_pfb(share_commitments=[]), 0),
        "MISMATCHED_COUNTS": (with_pfb(share_commitments=p.share_commitments + [bytes(32)]), 0),
        "INVALID_NAMESPACE": (with_pfb(namespaces=replaced(p.namespaces, 1, NS[1][1:])), 1),
        "RESERVED_NAMESPACE": (with_pfb(namespaces=replaced(p.namespaces, 0, bytes(28) + b"\x04")), 0),
        "INVALID_NAMESPACE_VERSION": (with_pfb(namespaces=replaced(p.namespaces, 1, b"\xff" + bytes(28))), 1),
        "UNSUPPORTED_SHARE_VERSION": (with_pfb(share_versions=[0, 1]), 1),
        "BAD_SIGNER": (with_pfb(signer="s"), 0),
        "BAD_COMMITMENT_LENGTH": (with_pfb(share_commitments=replaced(p.share_commitments, 1, bytes(31))), 1),
        "BLOB_NAMESPACE_VERSION_TOO_LARGE": (with_blob(namespace_version=256), 1),
        "BLOB_INVALID_NAMESPACE": (with_blob(namespace_version=1), 1),
        "BLOB_RESERVED_NAMESPACE": (with_blob(namespace_id=bytes(27) + b"\x04"), 1),
        "BLOB_INVALID_NAMESPACE_VERSION": (with_blob(namespace_version=255, namespace_id=bytes(28)), 1),
        "ZERO_BLOB_SIZE": (with_blob(data=b""), 1),
        "BLOB_UNSUPPORTED_SHARE_VERSION": (with_blob(share_version=1), 1),
        "SIZE_MISMATCH": (with_pfb(blob_sizes=[300, 21]), 1),
        "NAMESPACE_MISMATCH": (with_pfb(namespaces=replaced(p.namespaces, 1, NS[2])), 1),
        "NON_BLOB_TX_HAS_PFB": (bt.marshal_sdk_tx(URL_SEND, b"\x0a\x03abc",
                                                  extra_msgs=[(bt.URL_MSG_PAY_FOR_BLOBS, pfb)]), 1),
    }
    assert set(cases) == set(bt.KIND_NAMES)
    return cases


def word(kind: str, index: int = 0) -> int:
    return K[kind] | index << 8


def table_blocks():
    """Blocks of valid txs for the expected table: 1 blob; 5 blobs per tx; a tx
    with 70 blobs; several namespaces, so that plan order is not tx order;
    normal txs only; empty."""
    rng = random.Random(11)
    one_ns = dict(namespaces=NS[:1])
    return [
        [valid_tx(rng, 1)],
        [normal_tx(rng)] + [valid_tx(rng, 5) for _ in range(3)],
        [valid_tx(rng, 2, **one_ns), valid_tx(rng, 70, sizes=(1, 30, 478)), valid_tx(rng, 1)],
        [normal_tx(rng), normal_tx(rng)] + [valid_tx(rng, 3, namespaces=NS[::-1]) for _ in range(6)],
        [normal_tx(rng) for _ in range(4)],
        [],
    ]


def plans_table(blocks):
    """square.plan_native of every block as the planner's tables: (arena,
    records, blob_base, plans); a block plan_native refuses gets no plan."""
    rec = np.zeros(max(len(blocks), 1), sq.plan_record_dtype())
    parts, at, base, plans = [], 0, [0], []
    for i, txs in enumerate(blocks):
        try:
            k, plan = sq.plan_native(txs)
        except ValueError:
            k, plan = 0, None
            rec[i]["status"] = _abi.PLAN_LAYOUT
        plans.append(plan)
        nblob = 0 if plan is None else len(sq.plan_blobs(plan))
        if plan is not None:
            rec[i]["plan_off"], rec[i]["plan_bytes"], rec[i]["k"], rec[i]["nblob"] = at, plan.size, k, nblob
            parts.append(np.concatenate([plan, np.zeros(-plan.size % 16, np.uint8)]))
            at += parts[-1].size
        base.append(base[-1] + nblob)
    arena = np.concatenate(parts + [np.zeros(16, np.uint8)])
    return arena, rec[:len(blocks)], np.array(base, np.uint64), plans


def validate_host(blocks, arena=None, records=None, blob_base=None):
    """dagpu_blob_tx_validate_host over blocks of txs: (tx_status, block_status
    (n, 2), expected (rows, 32)) as uint32 / uint8 arrays."""
    L = _abi.lib()
    n = len(blocks)
    src, offs, ntx, lens = sq.pack_blocks(blocks)
    rows = int(blob_base[n]) if blob_base is not None else 0
    tx_status = np.full(max(lens.size, 1), 0xEEEEEEEE, np.uint32)
    block_status = np.full((max(n, 1), 2), 0xEEEEEEEE, np.uint32)
    expected = np.full((max(rows, 1), 32), 0xEE, np.uint8)
    rc = L.dagpu_blob_tx_validate_host(n, _abi.addr(src) if src.size else None, _abi.addr(offs), src.size,
                                       _abi.addr(ntx), _abi.addr(lens) if lens.size else None, _abi.addr(arena),
                                       0 if arena is None else arena.size, _abi.addr(records), _abi.addr(blob_base),
                                       _abi.addr(tx_status), _abi.addr(block_status), _abi.addr(expected))
    assert rc == 0, L.dagpu_last_error(None).decode()
    return tx_status[:lens.size], block_status[:n], expected[:rows]
