"""Tx signatures on the host: the mirror (blobtx.sign_doc_bytes, signer_of_tx,
check_signature) and the host executors of csrc/tx_sig.hpp
(dagpu_tx_sig_verify_host, dagpu_tx_signers_host) on hand-assembled SignDocs,
on one tx per kind, and on the batches the GPU tests use."""
import numpy as np
import pytest

from celestia_da import _abi, blobtx as bt, secp256k1 as ec

import tx_sig_cases as cases
from tx_sig_cases import K, word


def test_sign_doc_bytes_by_hand():
    body = b"\x0a\x04\x0a\x02/x"  # one message, Any {type_url "/x"}
    auth = b"\x12\x02hi"
    tx = b"\x0a" + bytes([len(body)]) + body + b"\x12" + bytes([len(auth)]) + auth + b"\x1a\x01s"
    want = b"\x0a\x06" + body + b"\x12\x04" + auth + b"\x1a\x03abc" + b"\x20\xac\x02"
    assert bt.sign_doc_bytes(tx, "abc", 300) == want
    # proto3 omission: account number 0, an empty chain id, an empty body, no auth_info
    assert bt.sign_doc_bytes(tx, "abc", 0) == b"\x0a\x06" + body + b"\x12\x04" + auth + b"\x1a\x03abc"
    assert bt.sign_doc_bytes(tx, "", 1) == b"\x0a\x06" + body + b"\x12\x04" + auth + b"\x20\x01"
    assert bt.sign_doc_bytes(b"\x12\x04" + auth, "abc", 2 ** 64 - 1) == \
        b"\x12\x04" + auth + b"\x1a\x03abc" + b"\x20" + b"\xff" * 9 + b"\x01"
    assert bt.sign_doc_bytes(b"\x0a\x00\x12\x00", b"c", 0) == b"\x1a\x01c"
    # a BlobTx signs its inner tx
    wrapped = cases.kind_cases()["blob tx"][0]
    inner = bt.unmarshal_blob_tx(wrapped)[0].tx
    assert bt.unmarshal_blob_tx(wrapped)[1] and bt.sign_doc_bytes(wrapped, "c", 5) == bt.sign_doc_bytes(inner, "c", 5)
    # a 200-byte body: a two-byte length
    long_body = b"\x0a\xc5\x01\x0a\xc2\x01" + b"/" * 194
    assert bt.sign_doc_bytes(b"\x0a\xc8\x01" + long_body, "", 0) == b"\x0a\xc8\x01" + long_body


def test_every_kind():
    names, txs, accts, table, words = cases.kind_block()
    for name, tx, acct, row, want in zip(names, txs, accts, table, words):
        kind, index = bt.check_signature(tx, cases.CHAIN_ID, int(acct), row.tobytes() if row[0] else None)
        assert kind | index << 8 == want, (name, kind, index)
    tx_status, block_status, signers = cases.verify_host([txs], accts, table)
    for name, got, want in zip(names, tx_status.tolist(), words):
        assert got == want, (name, got & 0xFF, got >> 8)
    rejecting = [i for i, w in enumerate(words) if w & 0xFF >= _abi.SIG_REJECTING]
    not_judged = sum(1 <= w & 0xFF < _abi.SIG_REJECTING for w in words)
    assert block_status.tolist() == [[rejecting[0], words[rejecting[0]], not_judged, 0]]
    assert {w & 0xFF for w in words} == set(_abi.SIG_KIND_NAMES)
    assert np.array_equal(signers, cases.mirror_signers([txs]))
    assert np.array_equal(signers, cases.signers_host([txs]))


def test_signer_records():
    c = cases.kind_cases()
    key, kind, sequence = bt.signer_of_tx(c["SIG_OK"][0])
    assert (key, kind, sequence) == (cases.PUBS[2], 0, 3)
    assert bt.signer_of_tx(c["blob tx"][0]) == (cases.PUBS[4], 0, 5)
    assert bt.signer_of_tx(c["SIG_NO_PUBKEY"][0]) == (bytes(33), K["SIG_NO_PUBKEY"], 3)
    assert bt.signer_of_tx(c["SIG_BAD_PUBKEY"][0]) == (bytes(33), K["SIG_BAD_PUBKEY"], 3)
    assert bt.signer_of_tx(c["SIG_UNSUPPORTED_MODE"][0]) == (bytes(33), K["SIG_UNSUPPORTED_MODE"], 3)
    assert bt.signer_of_tx(c["SIG_UNSUPPORTED_SIGNERS"][0]) == (bytes(33), K["SIG_UNSUPPORTED_SIGNERS"], 0)
    assert bt.signer_of_tx(c["SIG_BAD_LENGTH"][0]) == (cases.PUBS[2], K["SIG_BAD_LENGTH"], 3)
    # a wrong key in the tx is still the key the tx carries; the table does not change the record
    assert bt.signer_of_tx(c["wrong tx key"][0])[0] == ec.pubkey_of(cases.PRIVS[3])
    big = bt.marshal_sdk_tx(cases.URL_SEND, b"v", auth_info=bt.marshal_auth_info(cases.PUBS[0], 2 ** 64 - 1),
                            signatures=[bytes(64)])
    assert bt.signer_of_tx(big) == (cases.PUBS[0], 0, 2 ** 64 - 1)
    assert np.array_equal(cases.signers_host([[big]]), cases.mirror_signers([[big]]))


def test_chain_id_and_account_number():
    tx = cases.kind_cases()["SIG_OK"][0]
    assert bt.check_signature(tx, cases.CHAIN_ID, 7) == (0, 0)
    assert bt.check_signature(tx, cases.CHAIN_ID + "x", 7) == (K["SIG_MISMATCH"], 0)
    assert bt.check_signature(tx, "", 7) == (K["SIG_MISMATCH"], 0)
    accts = np.array([7], np.uint64)
    for chain, want in ((cases.CHAIN_ID, "SIG_OK"), (cases.CHAIN_ID + "x", "SIG_MISMATCH"), ("", "SIG_MISMATCH"),
                        ("c" * 64, "SIG_MISMATCH")):
        assert cases.verify_host([[tx]], accts, chain_id=chain)[0].tolist() == [word(want)], chain
    # a 64-byte chain id and a large account number, signed and verified
    long_chain = "z" * 64
    tx = cases.signed_tx(1, cases.URL_SEND, b"value", 2 ** 63 + 5, 9, chain_id=long_chain)
    assert bt.check_signature(tx, long_chain, 2 ** 63 + 5) == (0, 0)
    assert cases.verify_host([[tx]], np.array([2 ** 63 + 5], np.uint64), chain_id=long_chain)[0].tolist() == [0]
    assert cases.verify_host([[tx]], np.array([5], np.uint64), chain_id=long_chain)[0].tolist() == [word("SIG_MISMATCH")]


@pytest.mark.parametrize("batch", ["four", "long"])
def test_batches_host_equals_mirror(batch):
    blocks, accts = cases.batch_of_four() if batch == "four" else cases.long_tx_block()
    tx_status, block_status, signers = cases.verify_host(blocks, accts)
    want_tx, want_block = cases.mirror_words(blocks, accts)
    assert np.array_equal(tx_status, want_tx) and np.array_equal(block_status, want_block)
    assert np.array_equal(signers, cases.mirror_signers(blocks))
    if batch == "four":
        assert block_status.tolist() == [[40, word("SIG_MISMATCH"), 0, 0], [0xFFFFFFFF, 0, 0, 0],
                                         [3, word("SIG_BAD_LENGTH", 40), 1, 0], [0xFFFFFFFF, 0, 0, 0]]
        assert tx_status[270] == word("SIG_MISMATCH") and np.count_nonzero(tx_status) == 4
    else:
        assert not tx_status.any() and len(blocks[0][2]) > 70 * 1024


def test_refusals():
    L = _abi.lib()
    tx = cases.kind_cases()["SIG_OK"][0]
    accts = np.array([7], np.uint64)
    with pytest.raises(AssertionError, match="longer than 64"):
        cases.verify_host([[tx]], accts, chain_id="c" * 65)
    src = np.frombuffer(tx, np.uint8).copy()
    offs, ntx, lens = np.array([0, src.size], np.uint64), np.array([1], np.uint32), np.array([src.size], np.uint64)
    out = np.zeros(64, np.uint32)
    call = lambda **o: L.dagpu_tx_sig_verify_host(
        1, _abi.addr(src), o.get("offs", _abi.addr(offs)), src.size, _abi.addr(ntx), o.get("lens", _abi.addr(lens)),
        None, 0, o.get("accts", _abi.addr(accts)), None, o.get("status", _abi.addr(out)), _abi.addr(out[8:]),
        o.get("signers", _abi.addr(out[16:])))
    short = lens - 1
    for text, over in (("null", dict(offs=None)), ("null", dict(status=None)), ("null", dict(signers=None)),
                       ("null d_account_numbers", dict(accts=None)), ("tx_lens is required", dict(lens=None)),
                       ("add up", dict(lens=_abi.addr(short)))):
        assert call(**over) == _abi.ERR_ARG, text
        assert text in L.dagpu_last_error(None).decode(), (text, L.dagpu_last_error(None))
    assert call() == 0
    assert L.dagpu_tx_sig_verify_workspace_size(3, 10) == 32 + 16 + 32 * 3 + 16 * 10 + 64 + 136 * 10


# ---- tests/host/tx_sig_check.cpp: the executors' loops under the sanitizers -----------------------

def _build(tmp_path, name, flags):
    import os
    import subprocess

    from conftest import ROOT
    exe = str(tmp_path / name)
    # the headers' "#pragma unroll" is for hipcc
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", *flags, "-I", os.path.join(ROOT, "celestia-app_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "host", "tx_sig_check.cpp")], check=True, timeout=300)
    return exe


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]),
                                        ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined",
                                                       "-fno-sanitize-recover=all"])])
def test_tx_sig_check(tmp_path, name, flags):
    """The edge set through the raw loop, and every prefix and every
    substitution of 0x00, 0x7F, 0x80, 0xFF over one signed BlobTx through the
    tx loop, each in a heap buffer of exactly its length: a read at or past n
    is an AddressSanitizer report."""
    import struct
    import subprocess
    edge = cases.edge_cases()
    raw, acct = cases.kind_cases()["blob tx"][:2]
    chain = cases.CHAIN_ID.encode()
    blob = struct.pack("<I", len(edge)) + b"".join(p + d + s + struct.pack("<I", K[want]) for _, p, d, s, want in edge)
    blob += struct.pack("<I", len(raw)) + raw + struct.pack("<I", len(chain)) + chain + struct.pack("<Q", acct)
    path = tmp_path / "in.bin"
    path.write_bytes(blob)
    out = subprocess.run([_build(tmp_path, "tx_sig_check_" + name, flags), str(path)], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    f = dict(x.split("=") for x in out.stdout.split()[1:])
    assert int(f["raw"]) == len(edge) and int(f["valid"]) == 0 and int(f["prefixes"]) == len(raw) + 1
    assert int(f["substitutions"]) >= 3 * len(raw) and int(f["reached_curve"]) > 100
    # the program's words for the prefixes are the mirror's
    want = [bt.check_signature(raw[:i], cases.CHAIN_ID, acct) for i in range(len(raw) + 1)]
    assert [int(x) for x in f["prefix_words"].split(",")] == [k | i << 8 for k, i in want]
