#!/usr/bin/env python3
"""Writes tests/golden/secp256k1_openssl.json: ECDSA vectors over secp256k1
made by the local `openssl` command, an anchor that shares no arithmetic with
this project.  Per vector: `openssl ecparam -genkey`, `openssl ec -pubout
-conv_form compressed` (the key is the last 33 bytes of the DER
SubjectPublicKeyInfo) and `openssl dgst -sha256 -sign` (a DER SEQUENCE of two
INTEGERs, parsed here).  Each tuple {pubkey, msg, r, s} (hex) is stored twice:
under "openssl" as OpenSSL gave it (about half have s > n / 2, which
VerifySignature rejects as malleable) and under "low_s" with s normalised to
min(s, n - s).  The keys are fresh on every run, so the file changes; the tests
read the committed file and never call openssl.

usage: tools/make_secp256k1_vectors.py [count = 32]"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


def der_ints(der: bytes):
    """The two INTEGERs of SEQUENCE {INTEGER, INTEGER}."""
    def length(i):
        n = der[i]
        if n < 0x80:
            return n, i + 1
        k = n & 0x7F
        return int.from_bytes(der[i + 1:i + 1 + k], "big"), i + 1 + k
    assert der[0] == 0x30
    total, i = length(1)
    assert i + total == len(der)
    out = []
    for _ in range(2):
        assert der[i] == 0x02
        n, i = length(i + 1)
        out.append(int.from_bytes(der[i:i + n], "big"))
        i += n
    assert i == len(der)
    return out


def run(*args, **kw):
    return subprocess.run(args, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, **kw).stdout


def main():
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    raw, low = [], []
    with tempfile.TemporaryDirectory() as d:
        key, msgf = os.path.join(d, "key.pem"), os.path.join(d, "msg")
        for i in range(count):
            run("openssl", "ecparam", "-name", "secp256k1", "-genkey", "-noout", "-out", key)
            spki = run("openssl", "ec", "-in", key, "-pubout", "-conv_form", "compressed", "-outform", "DER")
            pub = spki[-33:]
            assert pub[0] in (2, 3)
            msg = (b"celestia-da secp256k1 vector %d;" % i) * (1 + i % 5) + bytes(range(i))
            with open(msgf, "wb") as f:
                f.write(msg)
            r, s = der_ints(run("openssl", "dgst", "-sha256", "-sign", key, msgf))
            for into, sv in ((raw, s), (low, min(s, N - s))):
                into.append({"pubkey": pub.hex(), "msg": msg.hex(), "r": "%064x" % r, "s": "%064x" % sv})
    path = os.path.join(ROOT, "tests", "golden", "secp256k1_openssl.json")
    with open(path, "w") as f:
        json.dump({"source": run("openssl", "version").decode().strip(), "openssl": raw, "low_s": low}, f, indent=1)
        f.write("\n")
    print(path, len(raw), "vectors,", sum(int(v["s"], 16) > N // 2 for v in raw), "with high s")


if __name__ == "__main__":
    main()
