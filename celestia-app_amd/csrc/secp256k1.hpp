// secp256k1.hpp -- ECDSA verification over secp256k1 as cosmos-sdk v0.46
// crypto/keys/secp256k1 PubKey.VerifySignature makes it, in one copy for the
// host (tx_sig_host.cpp) and the device (tx_sig.hip).  Plain arithmetic only
// (no HIP include); every function is marked for both sides when hipcc
// compiles it, and everything a lane runs is inlined: a call would put the
// caller's registers into scratch.
//
// Numbers are 8 x 32-bit limbs, little-endian, always fully reduced.  Both
// moduli have the form 2^256 - c (p: c = 2^32 + 977, two limbs; n: c has 129
// bits, five limbs), so one reduction serves both: a 512-bit product folds
// hi * c into lo three times (8 + CL limbs, then 9, then 8 and a carry), one
// more c is added for that carry, and one conditional subtraction finishes.
// Every limb index is a compile-time constant after unrolling: no per-lane
// array is indexed at run time (scalars are consumed by shifting them left).
//
// secp_verify, in this project's order (the reference reports every failure
// the same way):
//   kSigBadPubkey   prefix not 0x02 / 0x03, x >= p, or y = (x^3 + 7)^((p + 1) / 4)
//                   with y^2 != x^3 + 7
//   kSigOutOfRange  r = 0, r >= n or s = 0
//   kSigHighS       s > n / 2
//   kSigMismatch    with z = digest mod n, w = s^(n - 2), u1 = z w, u2 = r w:
//                   R = u1 G + u2 Q is infinity, or R.x mod n != r
// R is accumulated from the top: per 4 bits of the scalars, four times (double,
// add Q where the bit of u2 is set), then add (the nibble of u1) G from the
// table of 1 G .. 15 G (secp256k1_table.hpp, affine, in constant memory on the
// device).  An addition that does not apply is computed and dropped by an
// arithmetic select, so a wave never diverges on scalar bits.  Jacobian
// coordinates, Z = 0 is infinity; the mixed addition handles an infinite
// accumulator (the result is the operand), equal operands (the doubling; a
// rare divergent branch) and opposite operands (H = 0 makes Z3 = 0).  The
// final comparison needs no inversion: r Z^2 == X (mod p), and (r + n) Z^2 == X
// when r + n < p, as libsecp256k1 compares.
#pragma once
#include <stdint.h>

#include "secp256k1_table.hpp"

#if defined(__HIPCC__)
#define DAGPU_HD __host__ __device__
#else
#define DAGPU_HD
#endif
// forced only where a call would cost scratch: in device code
#if defined(__HIP_DEVICE_COMPILE__)
#define DAGPU_EC_INLINE inline __attribute__((always_inline))
#else
#define DAGPU_EC_INLINE inline
#endif

namespace dagpu {

enum : uint32_t {
  kSigOk = 0,
  kSigTxUndecodable = 1,
  kSigUnsupportedSigners = 2,
  kSigUnsupportedMode = 3,
  kSigUnsupportedPubkeyType = 4,
  kSigNoPubkey = 5,
  kSigBadPubkey = 16,
  kSigBadLength = 17,
  kSigOutOfRange = 18,
  kSigHighS = 19,
  kSigMismatch = 20,
};

static const uint32_t kSecpGHost[15][16] = {DAGPU_SECP_G_ROWS};
static const uint32_t kSecpExpHost[3][8] = {DAGPU_SECP_EXP_ROWS};
#if defined(__HIPCC__)
static __constant__ const uint32_t kSecpGDev[15][16] = {DAGPU_SECP_G_ROWS};
static __constant__ const uint32_t kSecpExpDev[3][8] = {DAGPU_SECP_EXP_ROWS};
#endif
// row i: (i + 1) G, x then y
DAGPU_HD DAGPU_EC_INLINE const uint32_t* secp_g_row(uint32_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
  return kSecpGDev[i];
#else
  return kSecpGHost[i];
#endif
}
enum : uint32_t { kSecpExpSqrt = 0, kSecpExpInvN = 1, kSecpExpInvP = 2 };
DAGPU_HD DAGPU_EC_INLINE uint32_t secp_exp_bit(uint32_t which, uint32_t bit) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (kSecpExpDev[which][bit >> 5] >> (bit & 31)) & 1;
#else
  return (kSecpExpHost[which][bit >> 5] >> (bit & 31)) & 1;
#endif
}

struct U256 {
  uint32_t v[8];
};

// modulus = 2^256 - c
struct SecpP {
  static constexpr int CL = 2;
  static constexpr uint32_t c[5] = {977u, 1u, 0u, 0u, 0u};
};
struct SecpN {
  static constexpr int CL = 5;
  static constexpr uint32_t c[5] = {0x2FC9BEBFu, 0x402DA173u, 0x50B75FC4u, 0x45512319u, 1u};
};
// n / 2, rounded down
struct SecpHalfN {
  static constexpr uint32_t v[8] = {0x681B20A0u, 0xDFE92F46u, 0x57A4501Du, 0x5D576E73u,
                                    0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x7FFFFFFFu};
};

// ---- 256-bit integers ---------------------------------------------------------------
DAGPU_HD DAGPU_EC_INLINE U256 u256_zero() {
  U256 r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = 0;
  return r;
}
DAGPU_HD DAGPU_EC_INLINE U256 u256_small(uint32_t x) {
  U256 r = u256_zero();
  r.v[0] = x;
  return r;
}
template <class M>
DAGPU_HD DAGPU_EC_INLINE U256 secp_c() {
  U256 r = u256_zero();
#pragma unroll
  for (int i = 0; i < M::CL; i++) r.v[i] = M::c[i];
  return r;
}
// 32 big-endian bytes
DAGPU_HD DAGPU_EC_INLINE U256 u256_from_be(const uint8_t* b) {
  U256 r;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint8_t* p = b + 28 - 4 * i;
    r.v[i] = (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
  }
  return r;
}
DAGPU_HD DAGPU_EC_INLINE void u256_to_be(const U256& a, uint8_t* b) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint8_t* p = b + 28 - 4 * i;
    p[0] = (uint8_t)(a.v[i] >> 24);
    p[1] = (uint8_t)(a.v[i] >> 16);
    p[2] = (uint8_t)(a.v[i] >> 8);
    p[3] = (uint8_t)a.v[i];
  }
}
// r = a + b, returns the carry; r may be a or b
DAGPU_HD DAGPU_EC_INLINE uint32_t u256_add(U256& r, const U256& a, const U256& b) {
  uint64_t k = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    k += (uint64_t)a.v[i] + b.v[i];
    r.v[i] = (uint32_t)k;
    k >>= 32;
  }
  return (uint32_t)k;
}
// r = a - b, returns the borrow
DAGPU_HD DAGPU_EC_INLINE uint32_t u256_sub(U256& r, const U256& a, const U256& b) {
  uint64_t k = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t d = (uint64_t)a.v[i] - b.v[i] - k;
    r.v[i] = (uint32_t)d;
    k = (d >> 32) & 1;
  }
  return (uint32_t)k;
}
DAGPU_HD DAGPU_EC_INLINE bool u256_is_zero(const U256& a) {
  uint32_t x = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) x |= a.v[i];
  return x == 0;
}
DAGPU_HD DAGPU_EC_INLINE bool u256_eq(const U256& a, const U256& b) {
  uint32_t x = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) x |= a.v[i] ^ b.v[i];
  return x == 0;
}
// a >= 2^256 - c
template <class M>
DAGPU_HD DAGPU_EC_INLINE bool secp_ge_mod(const U256& a) {
  U256 t;
  return u256_add(t, a, secp_c<M>()) != 0;
}
// mask all ones: b, else a
DAGPU_HD DAGPU_EC_INLINE U256 u256_select(const U256& a, const U256& b, uint32_t mask) {
  U256 r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = (a.v[i] & ~mask) | (b.v[i] & mask);
  return r;
}
// a << s, 1 <= s <= 31; returns the bits shifted out
DAGPU_HD DAGPU_EC_INLINE uint32_t u256_shl(U256& a, uint32_t s) {
  const uint32_t out = a.v[7] >> (32 - s);
#pragma unroll
  for (int i = 7; i > 0; i--) a.v[i] = a.v[i] << s | a.v[i - 1] >> (32 - s);
  a.v[0] <<= s;
  return out;
}

// ---- arithmetic mod 2^256 - c ----------------------------------------------------------
template <class M>
DAGPU_HD DAGPU_EC_INLINE U256 fe_add(const U256& a, const U256& b) {
  U256 s, e;
  const uint32_t k = u256_add(s, a, b);
  const uint32_t k2 = u256_add(e, s, secp_c<M>());
  return u256_select(s, e, (k | k2) ? 0xFFFFFFFFu : 0u);
}
template <class M>
DAGPU_HD DAGPU_EC_INLINE U256 fe_sub(const U256& a, const U256& b) {
  U256 d, e;
  const uint32_t k = u256_sub(d, a, b);
  u256_sub(e, d, secp_c<M>());
  return u256_select(d, e, k ? 0xFFFFFFFFu : 0u);
}
// out[NA + NB] = a[NA] * b[NB]
template <int NA, int NB>
DAGPU_HD DAGPU_EC_INLINE void mp_mul(uint32_t* out, const uint32_t* a, const uint32_t* b) {
#pragma unroll
  for (int i = 0; i < NA + NB; i++) out[i] = 0;
#pragma unroll
  for (int i = 0; i < NA; i++) {
    uint32_t carry = 0;
#pragma unroll
    for (int j = 0; j < NB; j++) {
      const uint64_t uv = (uint64_t)a[i] * b[j] + out[i + j] + carry;
      out[i + j] = (uint32_t)uv;
      carry = (uint32_t)(uv >> 32);
    }
    out[i + NB] = carry;
  }
}
// t[16] mod 2^256 - c
template <class M>
DAGPU_HD DAGPU_EC_INLINE U256 fe_reduce(const uint32_t* t) {
  constexpr int CL = M::CL;
  constexpr int W2 = (2 * CL > 8 ? 2 * CL : 8) + 1;
  uint32_t c[CL];
#pragma unroll
  for (int i = 0; i < CL; i++) c[i] = M::c[i];
  // round 1: a1[8 + CL] = lo + hi * c
  uint32_t a1[8 + CL];
  mp_mul<8, CL>(a1, t + 8, c);
  uint64_t k = 0;
#pragma unroll
  for (int i = 0; i < 8 + CL; i++) {
    k += (uint64_t)a1[i] + (i < 8 ? t[i] : 0u);
    a1[i] = (uint32_t)k;
    k >>= 32;
  }
  // round 2: a2 = a1.lo + a1.hi * c < 2^259: limb 8 is small, the limbs above it are zero
  uint32_t h2[2 * CL], a2[W2];
  mp_mul<CL, CL>(h2, a1 + 8, c);
  k = 0;
#pragma unroll
  for (int i = 0; i < W2; i++) {
    k += (uint64_t)(i < 8 ? a1[i] : 0u) + (i < 2 * CL ? h2[i] : 0u);
    a2[i] = (uint32_t)k;
    k >>= 32;
  }
  // rounds 3 and 4: fold limb 8, then the carry of that
  U256 r;
  uint32_t hi = a2[8];
#pragma unroll
  for (int round = 0; round < 2; round++) {
    uint64_t m = 0;
    k = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      if (i < CL) m += (uint64_t)hi * c[i];
      k += (uint64_t)(round == 0 ? a2[i] : r.v[i]) + (uint32_t)m;
      m >>= 32;
      r.v[i] = (uint32_t)k;
      k >>= 32;
    }
    hi = (uint32_t)k;
  }
  U256 e;
  const uint32_t ge = u256_add(e, r, secp_c<M>());
  return u256_select(r, e, ge ? 0xFFFFFFFFu : 0u);
}
template <class M>
DAGPU_HD DAGPU_EC_INLINE U256 fe_mul(const U256& a, const U256& b) {
  uint32_t t[16];
  mp_mul<8, 8>(t, a.v, b.v);
  return fe_reduce<M>(t);
}
template <class M>
DAGPU_HD DAGPU_EC_INLINE U256 fe_sqr(const U256& a) {
  return fe_mul<M>(a, a);
}
// a^e for the fixed exponent `which` of kSecpExp: square and multiply from the
// top bit; the branch on an exponent bit is uniform over the wave
template <class M>
DAGPU_HD DAGPU_EC_INLINE U256 fe_pow(const U256& a, uint32_t which) {
  U256 acc = u256_small(1);
#pragma unroll 1
  for (int i = 255; i >= 0; i--) {
    acc = fe_sqr<M>(acc);
    if (secp_exp_bit(which, (uint32_t)i)) acc = fe_mul<M>(acc, a);
  }
  return acc;
}

// ---- the curve y^2 = x^3 + 7 -------------------------------------------------------------
struct SecpJac {
  U256 x, y, z;  // z = 0: infinity
};
// dbl-2009-l (a = 0); infinity stays infinity (Z3 = 2 Y Z); no point has Y = 0
DAGPU_HD DAGPU_EC_INLINE void secp_dbl(SecpJac& r) {
  using F = SecpP;
  const U256 a = fe_sqr<F>(r.x);
  const U256 b = fe_sqr<F>(r.y);
  const U256 c = fe_sqr<F>(b);
  U256 d = fe_sqr<F>(fe_add<F>(r.x, b));
  d = fe_sub<F>(fe_sub<F>(d, a), c);
  d = fe_add<F>(d, d);
  const U256 e = fe_add<F>(fe_add<F>(a, a), a);
  const U256 f = fe_sqr<F>(e);
  const U256 z3 = fe_mul<F>(r.y, r.z);
  r.z = fe_add<F>(z3, z3);
  r.x = fe_sub<F>(f, fe_add<F>(d, d));
  U256 c8 = fe_add<F>(c, c);
  c8 = fe_add<F>(c8, c8);
  c8 = fe_add<F>(c8, c8);
  r.y = fe_sub<F>(fe_mul<F>(e, fe_sub<F>(d, r.x)), c8);
}
// r += (px, py), an affine point that is not infinity (madd-2007-bl); with skip
// (all ones) r stays as it is
DAGPU_HD DAGPU_EC_INLINE void secp_madd(SecpJac& r, const U256& px, const U256& py, uint32_t skip) {
  using F = SecpP;
  const uint32_t r_inf = u256_is_zero(r.z) ? 0xFFFFFFFFu : 0u;
  const U256 z1z1 = fe_sqr<F>(r.z);
  const U256 u2 = fe_mul<F>(px, z1z1);
  const U256 s2 = fe_mul<F>(py, fe_mul<F>(r.z, z1z1));
  const U256 h = fe_sub<F>(u2, r.x);
  U256 rr = fe_sub<F>(s2, r.y);
  if (!skip && !r_inf && u256_is_zero(h) && u256_is_zero(rr)) {  // the operands are equal
    secp_dbl(r);
    return;
  }
  rr = fe_add<F>(rr, rr);
  const U256 hh = fe_sqr<F>(h);
  U256 i4 = fe_add<F>(hh, hh);
  i4 = fe_add<F>(i4, i4);
  const U256 j = fe_mul<F>(h, i4);
  const U256 v = fe_mul<F>(r.x, i4);
  U256 x3 = fe_sub<F>(fe_sub<F>(fe_sqr<F>(rr), j), fe_add<F>(v, v));
  U256 yj = fe_mul<F>(r.y, j);
  yj = fe_add<F>(yj, yj);
  U256 y3 = fe_sub<F>(fe_mul<F>(rr, fe_sub<F>(v, x3)), yj);
  // opposite operands: h = 0 gives z3 = 0, infinity
  U256 z3 = fe_sub<F>(fe_sub<F>(fe_sqr<F>(fe_add<F>(r.z, h)), z1z1), hh);
  x3 = u256_select(x3, px, r_inf);
  y3 = u256_select(y3, py, r_inf);
  z3 = u256_select(z3, u256_small(1), r_inf);
  r.x = u256_select(x3, r.x, skip);
  r.y = u256_select(y3, r.y, skip);
  r.z = u256_select(z3, r.z, skip);
}

// x and y of the 33-byte compressed key; false: it is none
DAGPU_HD DAGPU_EC_INLINE bool secp_parse_pubkey(const uint8_t* pk33, U256& x, U256& y) {
  using F = SecpP;
  const uint8_t prefix = pk33[0];
  x = u256_from_be(pk33 + 1);
  if ((prefix != 2 && prefix != 3) || secp_ge_mod<F>(x)) return false;
  const U256 rhs = fe_add<F>(fe_mul<F>(fe_sqr<F>(x), x), u256_small(7));
  y = fe_pow<F>(rhs, kSecpExpSqrt);
  if (!u256_eq(fe_sqr<F>(y), rhs)) return false;
  const U256 neg = fe_sub<F>(u256_zero(), y);
  y = u256_select(y, neg, (y.v[0] & 1) != (uint32_t)(prefix & 1) ? 0xFFFFFFFFu : 0u);
  return true;
}

// kSigOk, kSigOutOfRange, kSigHighS or kSigMismatch for the key (qx, qy)
DAGPU_HD DAGPU_EC_INLINE uint32_t secp_verify_point(const uint8_t* z32, const uint8_t* r32, const uint8_t* s32,
                                                    const U256& qx, const U256& qy) {
  const U256 r = u256_from_be(r32), s = u256_from_be(s32);
  if (u256_is_zero(r) || secp_ge_mod<SecpN>(r) || u256_is_zero(s)) return kSigOutOfRange;
  {
    U256 half, t;
#pragma unroll
    for (int i = 0; i < 8; i++) half.v[i] = SecpHalfN::v[i];
    if (u256_sub(t, half, s)) return kSigHighS;  // n / 2 < s
  }
  U256 z = u256_from_be(z32);
  {
    U256 e;
    const uint32_t ge = u256_add(e, z, secp_c<SecpN>());
    z = u256_select(z, e, ge ? 0xFFFFFFFFu : 0u);
  }
  const U256 w = fe_pow<SecpN>(s, kSecpExpInvN);
  U256 u1 = fe_mul<SecpN>(z, w), u2 = fe_mul<SecpN>(r, w);
  SecpJac acc;
  acc.x = acc.y = acc.z = u256_zero();
#pragma unroll 1
  for (int nib = 0; nib < 64; nib++) {
#pragma unroll 1
    for (int t = 0; t < 5; t++) {
      U256 ax, ay;
      uint32_t skip;
      if (t < 4) {
        secp_dbl(acc);
        skip = u256_shl(u2, 1) ? 0u : 0xFFFFFFFFu;
        ax = qx;
        ay = qy;
      } else {
        const uint32_t d = u256_shl(u1, 4);
        skip = d ? 0u : 0xFFFFFFFFu;
        const uint32_t* row = secp_g_row(d ? d - 1 : 0);
#pragma unroll
        for (int i = 0; i < 8; i++) {
          ax.v[i] = row[i];
          ay.v[i] = row[8 + i];
        }
      }
      secp_madd(acc, ax, ay, skip);
    }
  }
  if (u256_is_zero(acc.z)) return kSigMismatch;
  const U256 zz = fe_sqr<SecpP>(acc.z);
  if (u256_eq(fe_mul<SecpP>(r, zz), acc.x)) return kSigOk;
  // R.x in [n, p) reduces to r = R.x - n: r + n < p
  U256 rn, n_, zero = u256_zero();
  u256_sub(n_, zero, secp_c<SecpN>());  // n = 2^256 - c
  if (u256_add(rn, r, n_) == 0 && !secp_ge_mod<SecpP>(rn) && u256_eq(fe_mul<SecpP>(rn, zz), acc.x)) return kSigOk;
  return kSigMismatch;
}

// the whole verification of one (digest, r, s, compressed key)
DAGPU_HD DAGPU_EC_INLINE uint32_t secp_verify(const uint8_t* z32, const uint8_t* r32, const uint8_t* s32,
                                              const uint8_t* pk33) {
  U256 qx, qy;
  if (!secp_parse_pubkey(pk33, qx, qy)) return kSigBadPubkey;
  return secp_verify_point(z32, r32, s32, qx, qy);
}

// i G for i >= 1 as 64 big-endian bytes x | y, by repeated addition and one
// inversion: what the table of secp256k1_table.hpp must hold (host only; the
// tests compare)
inline void secp_g_multiple(uint32_t i, uint8_t* out64) {
  using F = SecpP;
  U256 gx, gy;
  for (int q = 0; q < 8; q++) {
    gx.v[q] = kSecpGHost[0][q];
    gy.v[q] = kSecpGHost[0][8 + q];
  }
  SecpJac acc;
  acc.x = acc.y = acc.z = u256_zero();
  for (uint32_t q = 0; q < i; q++) secp_madd(acc, gx, gy, 0);
  const U256 zi = fe_pow<F>(acc.z, kSecpExpInvP);
  const U256 zi2 = fe_sqr<F>(zi);
  u256_to_be(fe_mul<F>(acc.x, zi2), out64);
  u256_to_be(fe_mul<F>(acc.y, fe_mul<F>(zi2, zi)), out64 + 32);
}

}  // namespace dagpu
