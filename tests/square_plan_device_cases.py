"""Blocks of txs for the device planner (csrc/square_plan.hpp: dagpu_square_plan_emulate_host
on the CPU, dagpu_square_plan_device on the GPU), beyond square_corpus.corpus():
txs built byte by byte against every rule of blob.UnmarshalBlobTx, and blocks at
the edges of the layout and of the planner's own chunking.  Each entry is
(name, txs, max_square_size); what is expected of an entry always comes from
the host planner (square.plan_native), never from here."""
import functools
import random

from celestia_da import shares as sh

from test_square_host import NS1, NS2, NS3, blob_txs, normal_txs, pfb_tx

# csrc/square_plan.hpp kSpLanes: txs per chunk of the append scan, PFBs per chunk
# of the PFB stream scan, lanes of the sorting network
SCAN_CHUNK = 256


def varint(v):
    return sh.put_uvarint(v)


def key(num, wt):
    return varint(num << 3 | wt)


def field(num, payload):
    return key(num, 2) + varint(len(payload)) + payload


def vfield(num, v):
    return key(num, 0) + varint(v)


def ns_id(ns):
    """The 28-byte ID of a 29-byte namespace of shares.py."""
    return bytes(ns)[1:]


def blob_msg(ident, data, share_version=None, ns_version=None, extra=b""):
    out = field(1, ident) + field(2, data)
    if share_version is not None:
        out += vfield(3, share_version)
    if ns_version is not None:
        out += vfield(4, ns_version)
    return out + extra


def blob_tx(inner, *blobs, type_id=b"BLOB", extra=b""):
    out = field(1, inner) if inner is not None else b""
    return out + b"".join(field(2, b) for b in blobs) + extra + field(3, type_id)


def good_blob_tx(rng, size=100, ns=NS2):
    return blob_tx(pfb_tx([size]), blob_msg(ns_id(ns), rng.randbytes(size)))


def tx_of_compact_shares(rng, shares):
    """One normal tx whose delimited bytes fill exactly `shares` compact shares to the last byte."""
    want = 474 + (shares - 1) * 478
    n = want - len(varint(want))
    while n + len(varint(n)) > want:
        n -= 1
    return rng.randbytes(n)


@functools.lru_cache(maxsize=None)
def crafted_txs():
    """(name, tx): single txs against the parser's rules."""
    rng = random.Random(99)
    ident = ns_id(NS1)
    data = rng.randbytes(300)
    inner = pfb_tx([300])
    good = blob_msg(ident, data)
    out = []
    for n in (1, 2, 7, 64, 1000):
        out.append((f"random_{n}", rng.randbytes(n)))
    out.append(("sdk_tx_shape", field(1, rng.randbytes(120)) + field(2, rng.randbytes(60)) + field(3, rng.randbytes(64))))
    out.append(("type_id_not_blob", blob_tx(inner, good, type_id=b"BLOC")))
    out.append(("type_id_short", blob_tx(inner, good, type_id=b"BLO")))
    out.append(("type_id_long", blob_tx(inner, good, type_id=b"BLOBS")))
    out.append(("no_blob", blob_tx(inner)))
    out.append(("ns_id_27", blob_tx(inner, blob_msg(ident[:27], data))))
    out.append(("ns_id_29", blob_tx(inner, blob_msg(ident + b"\x00", data))))
    out.append(("ns_id_missing", blob_tx(inner, field(2, data))))
    out.append(("one_bad_ns_id_of_two", blob_tx(inner, good, blob_msg(ident[:5], data))))
    out.append(("field_1_twice", field(1, rng.randbytes(50)) + blob_tx(inner, good)))
    out.append(("field_3_twice_last_wins", field(3, b"NOPE") + blob_tx(inner, good)))
    out.append(("field_3_twice_last_loses", blob_tx(inner, good) + field(3, b"NOPE")))
    out.append(("ns_twice_in_blob", blob_tx(inner, field(1, b"\x09" * 28) + good)))
    out.append(("unknown_wt0", blob_tx(inner, good, extra=vfield(9, 1 << 40))))
    out.append(("unknown_wt1", blob_tx(inner, good, extra=key(10, 1) + bytes(8))))
    out.append(("unknown_wt5", blob_tx(inner, good, extra=key(11, 5) + bytes(4))))
    out.append(("unknown_wt2", blob_tx(inner, good, extra=field(12, b"xyz"))))
    out.append(("unknown_in_blob", blob_tx(inner, blob_msg(ident, data, extra=key(10, 1) + bytes(8) + key(11, 5) + bytes(4)
                                                         + vfield(9, 5)))))
    out.append(("wt1_cut_short", blob_tx(inner, good) + key(10, 1) + bytes(7)))
    out.append(("wt5_cut_short", blob_tx(inner, good) + key(11, 5) + bytes(3)))
    out.append(("wire_type_3", blob_tx(inner, good, extra=key(9, 3))))
    out.append(("wire_type_4", blob_tx(inner, good, extra=key(9, 4))))
    out.append(("wire_type_6_in_blob", blob_tx(inner, blob_msg(ident, data, extra=key(9, 6)))))
    out.append(("field_number_0", blob_tx(inner, good, extra=b"\x02\x00")))
    out.append(("field_1_as_varint", vfield(1, 7) + blob_tx(None, good)))
    out.append(("share_version_as_bytes", blob_tx(inner, field(1, ident) + field(2, data) + field(3, b"\x00"))))
    out.append(("varint_10_bytes", blob_tx(inner, good, extra=key(9, 0) + b"\xff" * 9 + b"\x01")))
    out.append(("varint_11_bytes", blob_tx(inner, good, extra=key(9, 0) + b"\xff" * 10 + b"\x01")))
    out.append(("varint_cut_short", blob_tx(inner, good) + key(9, 0) + b"\xff"))
    out.append(("length_past_tx", field(1, inner) + field(2, good) + key(3, 2) + varint(5) + b"BLOB"))
    out.append(("length_far_past_tx", field(1, inner) + field(2, good) + key(3, 2) + varint((1 << 63) + 4) + b"BLOB"))
    out.append(("length_past_blob", blob_tx(inner, field(1, ident) + key(2, 2) + varint(len(data) + 1) + data)))
    out.append(("empty_inner_absent", blob_tx(None, good)))
    out.append(("empty_inner_present", blob_tx(b"", good)))
    out.append(("share_version_1", blob_tx(inner, blob_msg(ident, data, share_version=1))))
    out.append(("share_version_2_pow_32", blob_tx(inner, blob_msg(ident, data, share_version=1 << 32))))
    out.append(("share_version_300", blob_tx(inner, blob_msg(ident, data, share_version=300))))
    out.append(("namespace_version_1", blob_tx(inner, blob_msg(ident, data, ns_version=1))))
    out.append(("namespace_version_255", blob_tx(inner, blob_msg(b"\xff" * 28, data, ns_version=255))))
    out.append(("namespace_version_256", blob_tx(inner, blob_msg(ident, data, ns_version=256))))
    out.append(("empty_blob_data", blob_tx(inner, blob_msg(ident, b""))))
    out.append(("blob_data_absent", blob_tx(inner, field(1, ident))))
    out.append(("two_blobs_second_empty", blob_tx(inner, good, blob_msg(ns_id(NS3), b""))))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def parser_blocks():
    """Every crafted tx alone, in front of a good blob tx and behind one: a tx
    taken for the wrong kind changes the plan or the error."""
    rng = random.Random(5)
    good = good_blob_tx(rng)
    out = []
    for name, tx in crafted_txs():
        out.append((f"{name}_alone", [tx], 128))
        out.append((f"{name}_first", [tx, good], 128))
        out.append((f"{name}_last", [good, tx], 128))
    # a namespace without its 18 leading zeros, behind which a blob of subtree
    # width 2 (in a namespace above it) needs a padding share in that namespace
    bad_ns = b"\x00" + b"\x05" * 27 + b"\x01"
    wide = rng.randbytes(sh.available_bytes_from_sparse_shares(70))
    for first in (100, 479):
        out.append((f"bad_padding_namespace_{first}",
                    [blob_tx(pfb_tx([first, len(wide)]), blob_msg(bad_ns[1:], rng.randbytes(first)),
                             blob_msg(b"\x06" * 28, wide))], 128))
    out.append(("bad_namespace_no_padding",
                [blob_tx(pfb_tx([10, 10]), blob_msg(bad_ns[1:], rng.randbytes(10)),
                         blob_msg(b"\x00" * 18 + b"\x07" * 10, rng.randbytes(10)))], 128))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def layout_blocks():
    rng = random.Random(11)
    A = sh.available_bytes_from_sparse_shares
    out = []
    for shares in (64, 65, 128, 129):  # the subtree width steps
        out.append((f"blob_{shares}_shares", blob_txs([NS1], [[A(shares)]], rng), 128))
        out.append((f"blob_{shares}_shares_behind_small", blob_txs([NS1, NS2], [[10], [A(shares)]], rng), 128))
    # share indexes 127 | 128 and 16,383: the varint steps inside the IndexWrapper
    for first in (127, 128, 16383):
        out.append((f"blob_at_{first}", [tx_of_compact_shares(rng, first - 1)] + blob_txs([NS1], [[20]], rng), 128))
    out.append(("blob_at_16384_does_not_fit", [tx_of_compact_shares(rng, 16383)] + blob_txs([NS1], [[20]], rng), 128))
    # five blobs of one PFB out of namespace order; NS1 shared by three PFBs
    out.append(("unordered_pfb_shared_ns",
                blob_txs([NS3, NS1, NS2, NS1, NS3, NS1, NS1, NS2], [[700, 30, 2000, 500, 10], [90], [40, 1000]], rng), 128))
    for n in (3, 4, 5):  # the sorting network's padding
        out.append((f"{n}_blobs", blob_txs([NS3, NS2, NS1, NS2, NS1][:n], [[50 + 10 * i] for i in range(n)], rng), 128))
    for base in (SCAN_CHUNK, 2 * SCAN_CHUNK):
        for n in (base - 1, base, base + 1):
            out.append((f"{n}_txs", normal_txs(rng, n, 40), 128))
    for n in (SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1):
        nss = [(NS1, NS2, NS3)[rng.randrange(3)] for _ in range(n)]
        out.append((f"{n}_pfbs", blob_txs(nss, [[rng.choice([5, 480, 1500])] for _ in range(n)], rng), 128))
        out.append((f"{n}_txs_mixed", normal_txs(rng, n - 7, 30) + blob_txs([NS2] * 7, [[60]] * 7, rng), 128))
    out.append(("zero_length_txs_and_pfbs", [b"", b"", b"\x01", b""] + blob_txs([NS1, NS2], [[5], [6]], rng), 128))
    # first failures (max square size 2 or 4: 4 or 16 shares)
    small = blob_txs([NS1], [[10]], rng)[0]
    out.append(("normal_tx_does_not_fit", [rng.randbytes(100), rng.randbytes(100), rng.randbytes(2000)], 2))
    out.append(("blob_tx_does_not_fit", [rng.randbytes(100), small, blob_txs([NS2], [[9000]], rng)[0]], 4))
    out.append(("normal_behind_blob_tx", [rng.randbytes(100), small, rng.randbytes(10), small], 4))
    out.append(("behind_blob_tx_then_no_space", [rng.randbytes(100), small, rng.randbytes(10), rng.randbytes(9000)], 4))
    out.append(("no_space_then_behind_blob_tx", [rng.randbytes(100), blob_txs([NS2], [[9000]], rng)[0], rng.randbytes(10)],
                4))
    out.append(("no_space_tx_then_blob_tx", [rng.randbytes(9000), small, rng.randbytes(10)], 4))
    out.append(("behind_blob_tx_and_no_space_at_once", [small, rng.randbytes(9000)], 4))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def batches():
    """(name, blocks, max_square_size): several blocks in one call."""
    rng = random.Random(23)
    a = normal_txs(rng, 3, 100) + blob_txs([NS2, NS1], [[600], [70]], rng)
    b = blob_txs([NS1], [[100]], rng)
    rejected = [blob_txs([NS1], [[10]], rng)[0], rng.randbytes(5)]
    w1 = [rng.randbytes(20)]
    w2 = [rng.randbytes(700)]
    w8 = blob_txs([NS3], [[sh.available_bytes_from_sparse_shares(40)]], rng)
    return (("empty_between", [a, [], b], 128), ("rejected_between", [a, rejected, b], 128),
            ("widths_1_2_8", [w1, w2, w8, w2, w1], 128), ("all_empty", [[], []], 128))


def all_blocks():
    return parser_blocks() + layout_blocks()
