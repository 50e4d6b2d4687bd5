"""Keys, signed txs, blocks and helpers shared by test_secp256k1_host.py,
test_tx_sig_host.py and test_gpu_tx_sig_device.py: the OpenSSL fixture, the edge
set of the raw verification, one tx per kind of _abi.SIG_KIND_NAMES, and the
host executors (dagpu_secp256k1_verify_host, dagpu_tx_signers_host,
dagpu_tx_sig_verify_host) as functions.  Everything signed is made once and
cached at module scope: signing is pure Python."""
import functools
import hashlib
import json
import os
import random

import numpy as np

from celestia_da import _abi, blobtx as bt, secp256k1 as ec, square as sq

import blobtx_validate_cases as bcases

K = _abi.SIG_KINDS
CHAIN_ID = "celestia-test-1"
URL_SEND = "/cosmos.bank.v1beta1.MsgSend"
PRIVS = [0x1000003 * (i + 1) ** 5 + 0xC0FFEE for i in range(8)]
PUBS = [ec.pubkey_of(p) for p in PRIVS]
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "secp256k1_openssl.json")


def word(kind: str, index: int = 0) -> int:
    return K[kind] | index << 8


# ---- the raw verification -------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fixture_cases():
    """[(name, pubkey33, digest32, sig64, expected kind name)] from the OpenSSL
    fixture: every tuple as OpenSSL signed it and low-S normalised."""
    with open(FIXTURE) as f:
        d = json.load(f)
    out = []
    for group in ("openssl", "low_s"):
        for i, v in enumerate(d[group]):
            s = int(v["s"], 16)
            want = "SIG_HIGH_S" if s > ec.HALF_N else "SIG_OK"
            out.append((f"{group}[{i}]", bytes.fromhex(v["pubkey"]), hashlib.sha256(bytes.fromhex(v["msg"])).digest(),
                        bytes.fromhex(v["r"] + v["s"]), want))
    assert len(out) >= 48 and any(c[4] == "SIG_HIGH_S" for c in out) and any(c[4] == "SIG_OK" for c in out)
    return out


def _flip(b: bytes, at: int) -> bytes:
    return b[:at] + bytes([b[at] ^ 0x20]) + b[at + 1:]


def _be(v: int) -> bytes:
    return v.to_bytes(32, "big")


def half_n_signature():
    """(priv, digest, sig) with s = n / 2 exactly: for a chosen nonce k and
    digest z, s = (z + r d) / k holds for the private key d = (s k - z) / r."""
    k, z = 0x5EED, hashlib.sha256(b"s = n / 2").digest()
    r = ec.mul(k, ec.G)[0] % ec.N
    d = (ec.HALF_N * k - int.from_bytes(z, "big")) * pow(r, -1, ec.N) % ec.N
    sig = ec.sign_digest(d, z, k, low_s=False)
    assert int.from_bytes(sig[32:], "big") == ec.HALF_N
    return d, z, sig


@functools.lru_cache(maxsize=None)
def edge_cases():
    """The edge set of the raw call, same shape as fixture_cases()."""
    out = []
    z = hashlib.sha256(b"edge").digest()
    # Q = G and Q = -G put the doubling and the infinity inside the addition; 2 G is the first table hit
    for name, d in (("priv 1", 1), ("priv 2", 2), ("priv n - 1", ec.N - 1), ("priv", PRIVS[0])):
        for nonce in (1, 2, 7, ec.N - 1, 0xABCDEF0123456789):
            out.append((f"{name}, nonce {nonce:#x}", ec.pubkey_of(d), z, ec.sign_digest(d, z, nonce), "SIG_OK"))
    d, pub = PRIVS[1], PUBS[1]
    good = ec.sign_digest(d, z, 0x1234567)
    r, s = good[:32], good[32:]
    zero, big = bytes(32), b"\xff" * 32  # u1 = 0; a digest >= n
    out.append(("digest 0", pub, zero, ec.sign_digest(d, zero, 99), "SIG_OK"))
    out.append(("digest >= n", pub, big, ec.sign_digest(d, big, 99), "SIG_OK"))
    out.append(("digest n", pub, _be(ec.N), ec.sign_digest(d, _be(ec.N), 99), "SIG_OK"))
    out.append(("digest 0 against digest n", pub, zero, ec.sign_digest(d, _be(ec.N), 99), "SIG_OK"))
    out.append(("r = 0", pub, z, bytes(32) + s, "SIG_OUT_OF_RANGE"))
    out.append(("r = n", pub, z, _be(ec.N) + s, "SIG_OUT_OF_RANGE"))
    out.append(("r = 2^256 - 1", pub, z, big + s, "SIG_OUT_OF_RANGE"))
    out.append(("r = n - 1, wrong s", pub, z, _be(ec.N - 1) + s, "SIG_MISMATCH"))
    out.append(("s = 0", pub, z, r + bytes(32), "SIG_OUT_OF_RANGE"))
    out.append(("s = n / 2 + 1", pub, z, r + _be(ec.HALF_N + 1), "SIG_HIGH_S"))
    out.append(("s = n - s", pub, z, r + _be(ec.N - int.from_bytes(s, "big")), "SIG_HIGH_S"))
    out.append(("s = n", pub, z, r + _be(ec.N), "SIG_HIGH_S"))
    out.append(("s = n / 2, wrong", pub, z, r + _be(ec.HALF_N), "SIG_MISMATCH"))
    hd, hz, hsig = half_n_signature()
    out.append(("s = n / 2, valid", ec.pubkey_of(hd), hz, hsig, "SIG_OK"))
    for at in (0, 5, 13, 31):  # 8 positions over r, s, the digest and the key each
        out.append((f"r byte {at}", pub, z, _flip(r, at) + s, None))
        out.append((f"s byte {at}", pub, z, r + _flip(s, at), None))
        out.append((f"digest byte {at}", pub, _flip(z, at), good, "SIG_MISMATCH"))
        out.append((f"key byte {at + 1}", _flip(pub, at + 1), z, good, None))
    out.append(("key parity", bytes([pub[0] ^ 1]) + pub[1:], z, good, "SIG_MISMATCH"))
    out.append(("key prefix 4", b"\x04" + pub[1:], z, good, "SIG_BAD_PUBKEY"))
    out.append(("key prefix 0", b"\x00" + pub[1:], z, good, "SIG_BAD_PUBKEY"))
    out.append(("key x = p", b"\x02" + _be(ec.P), z, good, "SIG_BAD_PUBKEY"))
    out.append(("key x = 2^256 - 1", b"\x03" + big, z, good, "SIG_BAD_PUBKEY"))
    x = next(x for x in range(1, 100) if ec.decompress(b"\x02" + _be(x)) is None)
    out.append(("key x off the curve", b"\x02" + _be(x), z, good, "SIG_BAD_PUBKEY"))
    out.append(("bad key before bad r", b"\x04" + pub[1:], z, bytes(64), "SIG_BAD_PUBKEY"))
    # a flipped byte of r, s or the key: whatever the mirror says, but never OK
    done = []
    for name, p, dg, sig, want in out:
        if want is None:
            want = ec.verify_digest(p, dg, sig)
            assert want != "SIG_OK", name
        done.append((name, p, dg, sig, want))
    return done


def raw_arrays(cases):
    """(digests (n, 32), sigs (n, 64), pubkeys (n, 33)) uint8 arrays."""
    col = lambda i, w: np.frombuffer(b"".join(c[i] for c in cases), np.uint8).reshape(len(cases), w).copy()
    return col(2, 32), col(3, 64), col(1, 33)


def raw_host(cases):
    """dagpu_secp256k1_verify_host over cases: the status words."""
    L = _abi.lib()
    digests, sigs, pubkeys = raw_arrays(cases)
    status = np.full(len(cases), 0xEEEEEEEE, np.uint32)
    rc = L.dagpu_secp256k1_verify_host(len(cases), _abi.addr(digests), _abi.addr(sigs), _abi.addr(pubkeys),
                                       _abi.addr(status))
    assert rc == 0, L.dagpu_last_error(None).decode()
    return status


# ---- signed txs -----------------------------------------------------------------------------

def signed_tx(key: int, url: str, value: bytes, account_number: int, sequence: int, chain_id=CHAIN_ID,
              nonce: int = 0, auth_info=None, tx_pubkey="own") -> bytes:
    """A cosmos Tx around one message, signed by PRIVS[key] over its SignDoc.
    nonce: one of a few values, so that the nonce points come from the cache."""
    if auth_info is None:
        auth_info = bt.marshal_auth_info(PUBS[key] if tx_pubkey == "own" else tx_pubkey, sequence, fee=b"\x0a\x03fee")
    unsigned = bt.marshal_sdk_tx(url, value, auth_info=auth_info)
    sig = ec.sign(PRIVS[key], bt.sign_doc_bytes(unsigned, chain_id, account_number), 0x51ED + nonce % 16)
    return bt.marshal_sdk_tx(url, value, auth_info=auth_info, signatures=[sig])


def signed_blob_tx(rng, key: int, account_number: int, sequence: int, nblobs: int = 1, **kw) -> bytes:
    blobs = bcases.blobs_of(rng, nblobs, sizes=(1, 40, 100))
    inner = signed_tx(key, bt.URL_MSG_PAY_FOR_BLOBS, bcases.pfb_of(blobs).marshal(), account_number, sequence, **kw)
    return bt.marshal_blob_tx(inner, *blobs)


@functools.lru_cache(maxsize=None)
def kind_cases():
    """{name: (raw tx, account number, table key or None, expected word)}: one
    tx per kind and the variations the issue lists."""
    rng = random.Random(21)
    val = rng.randbytes(50)
    key, pub = 2, PUBS[2]
    good = signed_tx(key, URL_SEND, val, 7, 3)

    def resigned(auth_info, acct=7, **kw):
        return signed_tx(key, URL_SEND, val, acct, 3, auth_info=auth_info, **kw)

    def with_sig(tx, sigs):
        body, auth, _ = bt._tx_raw(tx)
        return bt._wrap(1, body) + bt._bytes_field(2, auth) + b"".join(bt._wrap(3, s) for s in sigs)

    sig = bt._tx_raw(good)[2][0]
    r, s = sig[:32], sig[32:]
    other_key = ec.pubkey_of(PRIVS[3])
    off_curve = b"\x02" + next(x for x in range(1, 100) if ec.decompress(b"\x02" + _be(x)) is None).to_bytes(32, "big")
    no_key = resigned(bt.marshal_auth_info(None, 3))
    wrong_tx_key = resigned(bt.marshal_auth_info(other_key, 3))
    cases = {
        "SIG_OK": (good, 7, None, word("SIG_OK")),
        "SIG_TX_UNDECODABLE": (b"\x0a\x05abc", 0, None, word("SIG_TX_UNDECODABLE")),
        "undecodable auth_info": (bt.marshal_sdk_tx(URL_SEND, val, auth_info=b"\x0a\x05abc", signatures=[sig]), 0,
                                  None, word("SIG_TX_UNDECODABLE")),
        "undecodable body": (bt._wrap(1, b"\x0a\x05abc") + bt._bytes_field(2, bt._tx_raw(good)[1]) + bt._wrap(3, sig),
                             0, None, word("SIG_TX_UNDECODABLE")),
        "SIG_UNSUPPORTED_SIGNERS": (resigned(bt.marshal_auth_info(pub, 3, signers=2)), 7, None,
                                    word("SIG_UNSUPPORTED_SIGNERS", 2)),
        "no signer_infos": (bt.marshal_sdk_tx(URL_SEND, val, signatures=[sig]), 7, None,
                            word("SIG_UNSUPPORTED_SIGNERS", 0)),
        "two signatures": (with_sig(good, [sig, sig]), 7, None, word("SIG_UNSUPPORTED_SIGNERS", 1)),
        "no signature": (with_sig(good, []), 7, None, word("SIG_UNSUPPORTED_SIGNERS", 1)),
        "SIG_UNSUPPORTED_MODE": (resigned(bt.marshal_auth_info(pub, 3, mode=127)), 7, None,
                                 word("SIG_UNSUPPORTED_MODE", 127)),
        "mode multi": (resigned(bt.marshal_auth_info(pub, 3, multi=True)), 7, None, word("SIG_UNSUPPORTED_MODE", 0)),
        "mode unspecified": (resigned(bt.marshal_auth_info(pub, 3, mode=0)), 7, None, word("SIG_UNSUPPORTED_MODE", 0)),
        "SIG_UNSUPPORTED_PUBKEY_TYPE": (resigned(bt.marshal_auth_info(pub, 3, type_url="/cosmos.crypto.ed25519.PubKey")),
                                        7, None, word("SIG_UNSUPPORTED_PUBKEY_TYPE")),
        "SIG_NO_PUBKEY": (no_key, 7, None, word("SIG_NO_PUBKEY")),
        "table key, none in the tx": (no_key, 7, pub, word("SIG_OK")),
        "SIG_BAD_PUBKEY": (resigned(bt.marshal_auth_info(pub[:32], 3)), 7, None, word("SIG_BAD_PUBKEY")),
        "key off the curve": (resigned(bt.marshal_auth_info(off_curve, 3)), 7, None, word("SIG_BAD_PUBKEY")),
        "bad key before bad length": (with_sig(resigned(bt.marshal_auth_info(off_curve, 3)), [sig[:63]]), 7, None,
                                      word("SIG_BAD_PUBKEY")),
        "bad table key": (good, 7, off_curve, word("SIG_BAD_PUBKEY")),
        "SIG_BAD_LENGTH": (with_sig(good, [sig + b"\x00"]), 7, None, word("SIG_BAD_LENGTH", 65)),
        "empty signature": (with_sig(good, [b""]), 7, None, word("SIG_BAD_LENGTH", 0)),
        "SIG_OUT_OF_RANGE": (with_sig(good, [bytes(32) + s]), 7, None, word("SIG_OUT_OF_RANGE")),
        "SIG_HIGH_S": (with_sig(good, [r + _be(ec.N - int.from_bytes(s, "big"))]), 7, None, word("SIG_HIGH_S")),
        "SIG_MISMATCH": (with_sig(good, [r + _flip(s, 9)]), 7, None, word("SIG_MISMATCH")),
        "wrong account number": (good, 8, None, word("SIG_MISMATCH")),
        "account number 0": (signed_tx(key, URL_SEND, val, 0, 3), 0, None, word("SIG_OK")),
        "right table key, wrong tx key": (wrong_tx_key, 7, pub, word("SIG_OK")),
        "wrong table key, right tx key": (good, 7, other_key, word("SIG_MISMATCH")),
        "wrong tx key": (wrong_tx_key, 7, None, word("SIG_MISMATCH")),
        "blob tx": (signed_blob_tx(rng, 4, 11, 5, nblobs=2), 11, None, word("SIG_OK")),
        "blob tx, wrong account": (signed_blob_tx(rng, 4, 11, 5), 12, None, word("SIG_MISMATCH")),
        "empty body": (bt._bytes_field(2, bt._tx_raw(good)[1]) + bt._wrap(3, ec.sign(
            PRIVS[key], bt._bytes_field(2, bt._tx_raw(good)[1]) + bt._bytes_field(3, CHAIN_ID.encode()), 0x51ED)), 0,
                       None, word("SIG_OK")),
    }
    assert {n for n in cases if n.startswith("SIG_")} == set(K)
    return cases


def kind_block():
    """kind_cases() as one block: (names, txs, account numbers, table (ntx, 33), words)."""
    cases = kind_cases()
    names = list(cases)
    table = np.zeros((len(names), 33), np.uint8)
    for i, n in enumerate(names):
        if cases[n][2] is not None:
            table[i] = np.frombuffer(cases[n][2], np.uint8)
    return (names, [cases[n][0] for n in names], np.array([cases[n][1] for n in names], np.uint64), table,
            [cases[n][3] for n in names])


@functools.lru_cache(maxsize=None)
def batch_of_four():
    """([300 signed txs mixing normal txs and BlobTxs, [], 7 txs, 5 txs], account
    numbers): the lanes cross a 256-lane workgroup and an empty block.  Normal
    txs come first in a block, as the planner wants them.  A few txs are wrong
    on purpose: the block words must name the lowest."""
    rng = random.Random(22)
    blocks, accts = [], []
    for size, nblob in ((300, 180), (0, 0), (7, 0), (5, 3)):
        txs = []
        for i in range(size):
            key, acct = rng.randrange(8), rng.randrange(1, 1 << 40)
            if i < size - nblob:
                txs.append(signed_tx(key, URL_SEND, rng.randbytes(rng.randrange(1, 200)), acct, i, nonce=i))
            else:
                txs.append(signed_blob_tx(rng, key, acct, i, nonce=i))
            accts.append(acct)
        blocks.append(txs)
    accts = np.array(accts, np.uint64)
    accts[40] += 1    # block 0, tx 40: SIG_MISMATCH
    accts[270] += 1   # block 0, tx 270, a BlobTx: SIG_MISMATCH, not the lowest
    body, auth, sigs = bt._tx_raw(blocks[2][3])
    blocks[2][3] = bt._wrap(1, body) + bt._bytes_field(2, auth) + bt._wrap(3, sigs[0][:40])  # BAD_LENGTH 40
    blocks[2][5] = bt.marshal_sdk_tx(URL_SEND, b"x", signatures=[bytes(64)])  # no signer_infos: not judged
    return blocks, accts


def long_tx_block():
    """One 70 KB non-blob tx among short ones: the streamed hash over more
    than a thousand SHA blocks, one lane diverging."""
    rng = random.Random(23)
    txs = [signed_tx(i % 8, URL_SEND, rng.randbytes(30 + i), 100 + i, i, nonce=i) for i in range(5)]
    txs.insert(2, signed_tx(5, URL_SEND, rng.randbytes(70 * 1024), 99, 1))
    return [txs], np.array([100, 101, 99, 102, 103, 104], np.uint64)


def mirror_words(blocks, accts, table=None, chain_id=CHAIN_ID):
    """check_signature over every tx: (tx words, block words (n, 4))."""
    words, block_words, g = [], [], 0
    for txs in blocks:
        lowest, not_judged = (0xFFFFFFFF, 0), 0
        for i, tx in enumerate(txs):
            row = None if table is None or table[g, 0] == 0 else table[g].tobytes()
            kind, index = bt.check_signature(tx, chain_id, int(accts[g]), row)
            words.append(kind | index << 8)
            if kind >= _abi.SIG_REJECTING and lowest[0] == 0xFFFFFFFF:
                lowest = (i, words[-1])
            not_judged += 1 <= kind < _abi.SIG_REJECTING
            g += 1
        block_words.append([lowest[0], lowest[1], not_judged, 0])
    return np.array(words, np.uint32), np.array(block_words, np.uint32).reshape(len(blocks), 4)


def mirror_signers(blocks):
    out = np.zeros((sum(len(b) for b in blocks), _abi.SIGNER_RECORD_BYTES), np.uint8)
    g = 0
    for txs in blocks:
        for tx in txs:
            key, kind, sequence = bt.signer_of_tx(tx)
            out[g, :33] = np.frombuffer(key, np.uint8)
            out[g, 33] = kind
            out[g, 40:48] = np.frombuffer(int(sequence).to_bytes(8, "little"), np.uint8)
            g += 1
    return out


def verify_host(blocks, accts, table=None, chain_id=CHAIN_ID):
    """dagpu_tx_sig_verify_host: (tx_status, block_status (n, 4), signers (ntx, 48))."""
    L = _abi.lib()
    n = len(blocks)
    src, offs, ntx, lens = sq.pack_blocks(blocks)
    chain = np.frombuffer(chain_id.encode() if isinstance(chain_id, str) else chain_id, np.uint8).copy()
    accts = np.ascontiguousarray(accts, np.uint64)
    tx_status = np.full(max(lens.size, 1), 0xEEEEEEEE, np.uint32)
    block_status = np.full((max(n, 1), 4), 0xEEEEEEEE, np.uint32)
    signers = np.full((max(lens.size, 1), _abi.SIGNER_RECORD_BYTES), 0xEE, np.uint8)
    rc = L.dagpu_tx_sig_verify_host(n, _abi.addr(src) if src.size else None, _abi.addr(offs), src.size, _abi.addr(ntx),
                                    _abi.addr(lens) if lens.size else None, _abi.addr(chain) if chain.size else None,
                                    chain.size, _abi.addr(accts) if accts.size else None,
                                    None if table is None else _abi.addr(table), _abi.addr(tx_status),
                                    _abi.addr(block_status), _abi.addr(signers))
    assert rc == 0, L.dagpu_last_error(None).decode()
    return tx_status[:lens.size], block_status[:n], signers[:lens.size]


def signers_host(blocks):
    L = _abi.lib()
    src, offs, ntx, lens = sq.pack_blocks(blocks)
    signers = np.full((max(lens.size, 1), _abi.SIGNER_RECORD_BYTES), 0xEE, np.uint8)
    rc = L.dagpu_tx_signers_host(len(blocks), _abi.addr(src) if src.size else None, _abi.addr(offs), src.size,
                                 _abi.addr(ntx), _abi.addr(lens) if lens.size else None, _abi.addr(signers))
    assert rc == 0, L.dagpu_last_error(None).decode()
    return signers[:lens.size]
