"""secp256k1 ECDSA as cosmos-sdk v0.46 crypto/keys/secp256k1 verifies it
(PubKey.VerifySignature over SHA-256 of the sign bytes), on plain Python
integers: the readable mirror of csrc/secp256k1.hpp, written independently of
it.  Points are affine (None is the point at infinity); a scalar multiplication
runs in Jacobian coordinates inside.

A verdict is one of the names of _abi.SIG_KIND_NAMES, checked in this order:
  SIG_BAD_PUBKEY    key length != 33, prefix not 0x02 / 0x03, x >= p, or
                    x^3 + 7 not a square
  SIG_BAD_LENGTH    len(sig) != 64
  SIG_OUT_OF_RANGE  r = 0, r >= n or s = 0
  SIG_HIGH_S        s > n / 2 (malleable)
  SIG_MISMATCH      R = (z/s) G + (r/s) Q is infinity, or R.x mod n != r
  SIG_OK
"""
from __future__ import annotations

import functools
import hashlib
from typing import Optional, Tuple

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
GX = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
GY = 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8
G = (GX, GY)
HALF_N = N >> 1

Point = Optional[Tuple[int, int]]


def add(a: Point, b: Point) -> Point:
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return x, (lam * (a[0] - x) - a[1]) % P


def _jac_dbl(p):
    x, y, z = p
    a, b = x * x % P, y * y % P
    c = b * b % P
    d = 2 * ((x + b) * (x + b) - a - c) % P
    e = 3 * a % P
    x3 = (e * e - 2 * d) % P
    return x3, (e * (d - x3) - 8 * c) % P, 2 * y * z % P


def _jac_add(p, q: Tuple[int, int]):
    """Jacobian p (z = 0: infinity) plus the affine point q."""
    x, y, z = p
    if z == 0:
        return q[0], q[1], 1
    zz = z * z % P
    h, r = (q[0] * zz - x) % P, (q[1] * zz * z - y) % P
    if h == 0:
        return _jac_dbl(p) if r == 0 else (1, 1, 0)
    hh = h * h % P
    v = x * hh % P
    x3 = (r * r - hh * h - 2 * v) % P
    return x3, (r * (v - x3) - y * hh * h) % P, z * h % P


def mul2(a: int, p: Point, b: int, q: Point) -> Point:
    """a p + b q: one ladder over the bits of both scalars (Jacobian inside,
    so that a multiplication costs one inversion, not one per step)."""
    table = (None, p, q, add(p, q))
    acc = (1, 1, 0)
    for i in range(max(a.bit_length(), b.bit_length()) - 1, -1, -1):
        acc = _jac_dbl(acc)
        t = table[(a >> i & 1) | (b >> i & 1) << 1]
        if t is not None:
            acc = _jac_add(acc, t)
    if acc[2] == 0:
        return None
    zi = pow(acc[2], -1, P)
    return acc[0] * zi * zi % P, acc[1] * zi * zi * zi % P


def mul(k: int, a: Point) -> Point:
    return mul2(k, a, 0, None)


@functools.lru_cache(maxsize=256)
def _base_mul(k: int) -> Point:
    return mul(k, G)


def compress(a: Tuple[int, int]) -> bytes:
    return bytes([2 + (a[1] & 1)]) + a[0].to_bytes(32, "big")


def decompress(pubkey33: bytes) -> Point:
    """The point of a 33-byte compressed key, or None when it is none."""
    if len(pubkey33) != 33 or pubkey33[0] not in (2, 3):
        return None
    x = int.from_bytes(pubkey33[1:], "big")
    if x >= P:
        return None
    rhs = (x * x * x + 7) % P
    y = pow(rhs, (P + 1) // 4, P)
    if y * y % P != rhs:
        return None
    return x, (y if (y & 1) == (pubkey33[0] & 1) else P - y)


def pubkey_of(priv: int) -> bytes:
    """The compressed public key of a private scalar in [1, n)."""
    q = _base_mul(priv % N)
    if q is None:
        raise ValueError("the private key is a multiple of n")
    return compress(q)


def verify_digest(pubkey33: bytes, digest32: bytes, sig: bytes) -> str:
    q = decompress(bytes(pubkey33))
    if q is None:
        return "SIG_BAD_PUBKEY"
    if len(sig) != 64:
        return "SIG_BAD_LENGTH"
    r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
    if r == 0 or r >= N or s == 0:
        return "SIG_OUT_OF_RANGE"
    if s > HALF_N:
        return "SIG_HIGH_S"
    z = int.from_bytes(digest32, "big") % N
    w = pow(s, -1, N)
    pt = mul2(z * w % N, G, r * w % N, q)
    if pt is None or pt[0] % N != r:
        return "SIG_MISMATCH"
    return "SIG_OK"


def verify(pubkey33: bytes, msg: bytes, sig: bytes) -> str:
    return verify_digest(pubkey33, hashlib.sha256(bytes(msg)).digest(), sig)


def sign_digest(priv: int, digest32: bytes, nonce: int, low_s: bool = True) -> bytes:
    k = nonce % N
    pt = _base_mul(k)
    if k == 0 or pt is None:
        raise ValueError("bad nonce")
    r = pt[0] % N
    s = pow(k, -1, N) * (int.from_bytes(digest32, "big") + r * priv) % N
    if r == 0 or s == 0:
        raise ValueError("bad nonce")
    if low_s and s > HALF_N:
        s = N - s
    return r.to_bytes(32, "big") + s.to_bytes(32, "big")


def sign(priv: int, msg: bytes, nonce: int) -> bytes:
    """r || s over SHA-256(msg) with an explicit nonce (tests: deterministic
    vectors; never sign anything real this way), normalised to low S."""
    return sign_digest(priv, hashlib.sha256(bytes(msg)).digest(), nonce)
