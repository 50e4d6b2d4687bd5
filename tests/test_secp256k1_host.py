"""secp256k1 ECDSA on the host: the Python mirror (celestia_da/secp256k1.py) and
the host executor of csrc/secp256k1.hpp (dagpu_secp256k1_verify_host) against
the OpenSSL fixture (tests/golden/secp256k1_openssl.json, made by
tools/make_secp256k1_vectors.py), against known constants, and against each
other over the edge set of tx_sig_cases.edge_cases()."""
import hashlib

import numpy as np

from celestia_da import _abi, secp256k1 as ec

import tx_sig_cases as cases
from tx_sig_cases import K


def test_known_constants():
    # SEC 2 v2, section 2.4.1: G; 2 G as every published table has it
    assert ec.pubkey_of(1).hex() == "0279be667ef9dcbbac55a06295ce870b07029bfcdb2dce28d959f2815b16f81798"
    assert ec.pubkey_of(2).hex() == "02c6047f9441ed7d6d3045406e95c07cd85c778e4b8cef3ca7abac09b95c709ee5"
    assert ec.mul(ec.N, ec.G) is None and ec.mul(ec.N - 1, ec.G) == (ec.GX, ec.P - ec.GY)
    assert ec.add(ec.G, ec.mul(ec.N - 1, ec.G)) is None
    assert (ec.GY * ec.GY - ec.GX ** 3 - 7) % ec.P == 0
    assert ec.decompress(ec.pubkey_of(2)) == ec.mul(2, ec.G) == ec.add(ec.G, ec.G)


def test_mirror_agrees_with_openssl():
    for name, pub, digest, sig, want in cases.fixture_cases():
        assert ec.verify_digest(pub, digest, sig) == want, name


def test_host_executor_agrees_with_openssl():
    fx = cases.fixture_cases()
    got = cases.raw_host(fx)
    assert got.tolist() == [K[c[4]] for c in fx]
    assert set(got.tolist()) == {K["SIG_OK"], K["SIG_HIGH_S"]}


def test_sign_is_low_s_and_verifies():
    d = cases.PRIVS[5]
    for i in range(6):
        msg = b"message %d" % i
        sig = ec.sign(d, msg, 1000 + i)
        assert int.from_bytes(sig[32:], "big") <= ec.HALF_N
        assert ec.verify(ec.pubkey_of(d), msg, sig) == "SIG_OK"
        assert ec.verify(ec.pubkey_of(d), msg + b"!", sig) == "SIG_MISMATCH"
        assert ec.verify_digest(ec.pubkey_of(d), hashlib.sha256(msg).digest(), sig[:63]) == "SIG_BAD_LENGTH"


def test_g_table():
    """The committed table of 1 G .. 15 G, and the same multiples from the
    library's own point arithmetic, equal the mirror's."""
    L = _abi.lib()
    want = b"".join(x.to_bytes(32, "big") + y.to_bytes(32, "big") for x, y in (ec.mul(i, ec.G) for i in range(1, 16)))
    for recompute in (0, 1):
        out = np.zeros(15 * 64, np.uint8)
        assert L.dagpu_secp256k1_g_table(_abi.addr(out), recompute) == 0
        assert out.tobytes() == want, recompute


def test_edge_set():
    edge = cases.edge_cases()
    for name, pub, digest, sig, want in edge:
        assert ec.verify_digest(pub, digest, sig) == want, name
    got = cases.raw_host(edge)
    for (name, *_, want), word in zip(edge, got.tolist()):
        assert word == K[want], (name, word)
    assert {c[4] for c in edge} == {"SIG_OK", "SIG_BAD_PUBKEY", "SIG_OUT_OF_RANGE", "SIG_HIGH_S", "SIG_MISMATCH"}


def test_half_n_is_accepted():
    d, z, sig = cases.half_n_signature()
    assert ec.verify_digest(ec.pubkey_of(d), z, sig) == "SIG_OK"
    up = sig[:32] + (ec.HALF_N + 1).to_bytes(32, "big")
    assert ec.verify_digest(ec.pubkey_of(d), z, up) == "SIG_HIGH_S"


def test_raw_call_refusals():
    L = _abi.lib()
    buf = np.zeros(64, np.uint8)
    assert L.dagpu_secp256k1_verify_host(0, None, None, None, None) == 0
    assert L.dagpu_secp256k1_verify_host(1, None, _abi.addr(buf), _abi.addr(buf), _abi.addr(buf)) == _abi.ERR_ARG
    assert L.dagpu_secp256k1_g_table(None, 0) == _abi.ERR_ARG
