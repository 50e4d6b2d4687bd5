// proof_verify.hip -- batched proof verification on gfx950.
//
//   nmt Proof.VerifyInclusion (nmt v0.20.0, IgnoreMaxNamespace; celestia-core
//   ShareProof.VerifyProof) for many proofs: a leaf pass (one lane per proven
//   leaf) and a fold pass (one lane per proof);
//   crypto/merkle Proof.Verify (celestia-core RowProof.Validate) for many
//   proofs: one lane per proof;
//   nmt Proof.VerifyNamespace (presence, absence and empty proofs; rules of
//   include/dagpu.h, specification dagpu_nmt_verify_namespace): the same two
//   passes instantiated with NS = true -- 9-word descriptors, an absence
//   proof's one leaf record copied from its leaf hash, the empty-form decision
//   against the root, and the completeness test where a proof node is popped.
//
// The specification is the library's own host verifiers
// (dagpu_nmt_verify_inclusion / dagpu_merkle_verify, trees.cpp): the fold walks
// the same tree of [0, est) in the same order with an explicit stack, and every
// status equals what the host function returns for that proof.
//
// Every offset and count a kernel reads was checked on the host (trees.cpp
// pv_check_*) against the buffer totals before the launch; loops are bounded
// by those counts.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dagpu.h"
#include "forest.hpp"
#include "nmt_node.hpp"
#include "proof_verify.hpp"
#include "sha256.hpp"

namespace dagpu {

namespace {

// 29-B namespace at any alignment -> 8 little-endian dwords, zero padded
__device__ __forceinline__ void load_ns29(const uint8_t* p, uint32_t (&w)[8]) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; b++)
      if (4 * j + b < kNsSize) v |= (uint32_t)p[4 * j + b] << (8 * b);
    w[j] = v;
  }
}

__device__ __forceinline__ void load_bytes32(const uint8_t* p, uint32_t (&w)[8]) {
#pragma unroll
  for (int j = 0; j < 8; j++)
    w[j] = (uint32_t)p[4 * j] | ((uint32_t)p[4 * j + 1] << 8) | ((uint32_t)p[4 * j + 2] << 16) |
           ((uint32_t)p[4 * j + 3] << 24);
}

// packed 90-B node at any alignment -> register form of nmt_node.hpp
__device__ __forceinline__ void load_node90(const uint8_t* p, uint32_t (&mn)[8], uint32_t (&mx)[8],
                                            uint32_t (&dg)[8]) {
  load_ns29(p, mn);
  load_ns29(p + kNsSize, mx);
  load_bytes32(p + 2 * kNsSize, dg);
}

__device__ __forceinline__ void load_q(const uint8_t* p, uint32_t (&d)[8]) {
  const uint4* q = (const uint4*)p;
  const uint4 x0 = q[0], x1 = q[1];
  d[0] = x0.x; d[1] = x0.y; d[2] = x0.z; d[3] = x0.w;
  d[4] = x1.x; d[5] = x1.y; d[6] = x1.z; d[7] = x1.w;
}

__device__ __forceinline__ void store_q(uint8_t* p, const uint32_t (&d)[8]) {
  uint4* q = (uint4*)p;
  q[0] = make_uint4(d[0], d[1], d[2], d[3]);
  q[1] = make_uint4(d[4], d[5], d[6], d[7]);
}

// Byte p of the message 0x00 | ns (when off == 30) | data | SHA padding.
__device__ __forceinline__ uint32_t pv_msg_byte(const uint8_t* ns, const uint8_t* data, long off, long mlen,
                                                long tot, long p) {
  if (p == 0) return 0x00u;
  if (p < off) return ns[p - 1];
  if (p < mlen) return data[p - off];
  if (p == mlen) return 0x80u;
  if (p >= tot - 8) return (uint32_t)(((uint64_t)mlen * 8u) >> (8 * (tot - 1 - p))) & 0xFFu;
  return 0u;
}

// SHA-256 of 0x00 | ns? | data for any length and alignment (byte loads).
__device__ __forceinline__ void pv_sha_generic(const uint8_t* ns, const uint8_t* data, long dlen,
                                               uint32_t (&st)[8]) {
  const long off = ns ? 1 + kNsSize : 1;
  const long mlen = off + dlen;
  const long nblk = (mlen + 8) / 64 + 1;
  const long tot = nblk * 64;
  sha256_init(st);
#pragma unroll 1
  for (long b = 0; b < nblk; b++) {
    uint32_t m[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const long p = 64 * b + 4 * j;
      m[j] = (pv_msg_byte(ns, data, off, mlen, tot, p) << 24) | (pv_msg_byte(ns, data, off, mlen, tot, p + 1) << 16) |
             (pv_msg_byte(ns, data, off, mlen, tot, p + 2) << 8) | pv_msg_byte(ns, data, off, mlen, tot, p + 3);
    }
    sha256_compress(st, m);
  }
}

// share_leaf_sha256 (nmt_node.hpp) with the prefix words taken from the proof's
// namespace nw (8 dwords, zero padded) instead of share[0:29]: 16-B loads, one
// v_perm per message word, 9 compressions.
__device__ __forceinline__ void pv_share_leaf_sha256(const uint4* src, const uint32_t (&nw)[8],
                                                     uint32_t (&st)[8]) {
  uint4 cur[8];
  auto stage = [&](int sg) {
#pragma unroll
    for (int q = 0; q < 8; q++) cur[q] = src[8 * sg + q];
  };
  auto mid_block = [&](const uint4& u0, const uint4& u1, const uint4& u2, const uint4& u3, const uint4& u4) {
    const uint32_t d[20] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w, u2.x, u2.y,
                            u2.z, u2.w, u3.x, u3.y, u3.z, u3.w, u4.x, u4.y, u4.z, u4.w};
    uint32_t m[16];
#pragma unroll
    for (int j = 0; j < 16; j++) m[j] = __builtin_amdgcn_perm(d[j], d[j + 1], 0x06070001u);
    sha256_compress(st, m);
  };
  sha256_init(st);
  stage(0);
  {  // block 0: 0x00 | ns(29) | share[0:34]
    uint32_t m[16];
    const uint4 q0v = cur[0], q1v = cur[1], q2v = cur[2];
    const uint32_t d[12] = {q0v.x, q0v.y, q0v.z, q0v.w, q1v.x, q1v.y,
                            q1v.z, q1v.w, q2v.x, q2v.y, q2v.z, q2v.w};
#pragma unroll
    for (int j = 8; j < 16; j++) m[j] = __builtin_amdgcn_perm(d[j - 8], d[j - 7], 0x06070001u);
    const uint32_t m7lo = __builtin_amdgcn_perm(d[0], d[0], (PZ << 24) | (PZ << 16) | 0x0001u);
    m[0] = __builtin_amdgcn_perm(nw[0], nw[0], (PZ << 24) | 0x000102u);
#pragma unroll
    for (int j = 1; j <= 6; j++) m[j] = __builtin_amdgcn_perm(nw[j - 1], nw[j], 0x07000102u);
    m[7] = __builtin_amdgcn_perm(nw[6], nw[7], (0x0700u << 16) | (PZ << 8) | PZ) | m7lo;
    sha256_compress(st, m);
  }
  mid_block(cur[2], cur[3], cur[4], cur[5], cur[6]);  // block 1
  uint4 prev0 = cur[6], prev1 = cur[7];
#pragma unroll 1
  for (int s2 = 1; s2 <= 3; s2++) {  // blocks 2 s2 and 2 s2 + 1
    stage(s2);
    mid_block(prev0, prev1, cur[0], cur[1], cur[2]);
    mid_block(cur[2], cur[3], cur[4], cur[5], cur[6]);
    prev0 = cur[6];
    prev1 = cur[7];
  }
  {  // block 8: share[482:512] | 0x80 | zeros | bit length
    uint32_t m[16];
    const uint32_t d[8] = {prev0.x, prev0.y, prev0.z, prev0.w, prev1.x, prev1.y, prev1.z, prev1.w};
#pragma unroll
    for (int j = 0; j < 7; j++) m[j] = __builtin_amdgcn_perm(d[j], d[j + 1], 0x06070001u);
    m[7] = __builtin_amdgcn_perm(d[7], d[7], (0x0607u << 16) | (PZ << 8) | PZ) | 0x8000u;
#pragma unroll
    for (int j = 8; j < 15; j++) m[j] = 0u;
    m[15] = 542u * 8u;
    sha256_compress_t<true>(st, m);
  }
}

// proof of leaf record g: largest i with rec_off[i] <= g
__device__ __forceinline__ long pv_find(const int64_t* off, long n, long g) {
  long lo = 0, hi = n;  // off[lo] <= g < off[hi]
  while (hi - lo > 1) {
    const long mid = (lo + hi) >> 1;
    if (off[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// RFC-6962 inner node SHA256(0x01 | l | r); l, r, out in memory byte order
__device__ __forceinline__ void pv_rfc_inner(const uint32_t (&l)[8], const uint32_t (&r)[8], uint32_t (&out)[8]) {
  uint32_t st[8];
  sha256_init(st);
  uint32_t m[16];
  // bytes: 0x01 | l[0..31] | r[0..30]   then   r[31] | 0x80 | zeros | length
  m[0] = __builtin_amdgcn_perm(l[0], l[0], (PZ << 24) | 0x000102u) | 0x01000000u;
#pragma unroll
  for (int j = 1; j < 8; j++) m[j] = __builtin_amdgcn_perm(l[j - 1], l[j], 0x07000102u);
  m[8] = __builtin_amdgcn_perm(l[7], r[0], 0x07000102u);
#pragma unroll
  for (int j = 1; j < 8; j++) m[8 + j] = __builtin_amdgcn_perm(r[j - 1], r[j], 0x07000102u);
  sha256_compress(st, m);
  m[0] = (r[7] & 0xFF000000u) | 0x00800000u;
#pragma unroll
  for (int j = 1; j < 15; j++) m[j] = 0u;
  m[15] = 65u * 8u;
  sha256_compress(st, m);
#pragma unroll
  for (int j = 0; j < 8; j++) out[j] = bswap32(st[j]);
}

}  // namespace

// ---------------------------------------------------------------------------
// Leaf pass: one lane per proven leaf; record ns | ns | SHA256(0x00 | ns | leaf)
// with ns the namespace the proof claims.
// ---------------------------------------------------------------------------
template <bool NS>
__global__ __launch_bounds__(256) void pv_nmt_leaf_kernel(PvNmtArgs a, long n_records) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= n_records) return;
  const long i = pv_find(a.rec_off, a.n, g);
  const int64_t* d = a.desc + i * (NS ? kPvDescNmtNs : kPvDescNmt);
  if constexpr (NS) {
    if (d[8] >= 0) {  // absence: the one record is the proof's leaf hash, nothing is hashed
      uint32_t mn[8], mx[8], dg[8];
      load_node90(a.leaf_hashes + d[8] * kNodeSize, mn, mx, dg);
      uint8_t* o = a.recs + g * kRecNmt;
      store_q(o, mn); store_q(o + 32, mx); store_q(o + 64, dg);
      return;
    }
  }
  const long leaf = d[3] + (g - a.rec_off[i]);
  const uint8_t* nsp = a.ns + d[6] * kNsSize;
  const uint8_t* src = a.leaves + leaf * a.leaf_len;
  uint32_t nw[8], st[8];
  load_ns29(nsp, nw);
  if (a.fast512) {
    pv_share_leaf_sha256((const uint4*)src, nw, st);
  } else {
    pv_sha_generic(nsp, src, a.leaf_len, st);
  }
  uint4* o = (uint4*)(a.recs + g * kRecNmt);
  o[0] = make_uint4(nw[0], nw[1], nw[2], nw[3]);
  o[1] = make_uint4(nw[4], nw[5], nw[6], nw[7]);
  o[2] = o[0];
  o[3] = o[1];
  o[4] = make_uint4(bswap32(st[0]), bswap32(st[1]), bswap32(st[2]), bswap32(st[3]));
  o[5] = make_uint4(bswap32(st[4]), bswap32(st[5]), bswap32(st[6]), bswap32(st[7]));
}

// ---------------------------------------------------------------------------
// Fold pass: one lane per proof.  The recursion of the host verifier's root_of
// over the complete tree [0, 2^H) runs as a state machine: the subtree in hand
// is (lo, h); a finished left child is parked until its sibling is done.  Parked
// proof nodes are kept as their index (LDS, one int per height and lane), parked
// computed nodes go to the proof's slice of the record stack in the workspace.
// A lane that has both children in registers waits until every live lane of the
// wave does, so the node hash runs with all of them at once.
// ---------------------------------------------------------------------------
enum { kPvEval = 0, kPvAscend = 1, kPvHash = 2, kPvTail = 3 };

// NS: Proof.VerifyNamespace.  A proof node popped for a subtree left of the range
// must have max < nid, one popped right of it (the tail included) nid < min; nid
// is re-read from the namespace table at each pop rather than kept live.
template <bool NS>
__device__ __forceinline__ bool pv_incomplete(const uint8_t* nsp, bool left, const uint32_t (&mn)[8],
                                              const uint32_t (&mx)[8]) {
  if constexpr (!NS) return false;
  uint32_t nid[8];
  load_ns29(nsp, nid);
  return left ? !ns_less(mx, nid) : !ns_less(nid, mn);
}

template <bool NS>
__global__ __launch_bounds__(kPvFoldLanes) void pv_nmt_fold_kernel(PvNmtArgs a) {
  __shared__ int32_t s_ref[kPvMaxHeight + 2][kPvFoldLanes];  // [height][lane]: node index or -1
  const int lane = threadIdx.x;
  const long i = (long)blockIdx.x * kPvFoldLanes + lane;
  bool done = i >= a.n;
  int32_t result = DAGPU_ERR_PROOF;
  int64_t start = 0, end = 1, nl = 0, nn = 0, node_off = 0, rec0 = 0, cs0 = 0, root_ix = 0;
  int depth = 0;
  const uint8_t* nsp = a.ns;
  if (!done) {
    const int64_t* d = a.desc + i * (NS ? kPvDescNmtNs : kPvDescNmt);
    start = d[0]; end = d[1]; nl = d[2]; nn = d[4]; node_off = d[5]; root_ix = d[7];
    rec0 = a.rec_off[i];
    cs0 = a.cs_off[i];
    depth = (int)(a.cs_off[i + 1] - cs0);
    // a range the host verifier rejects has no records: DAGPU_ERR_PROOF
    if (depth == 0) done = true;
    if constexpr (NS) {
      nsp = a.ns + d[6] * kNsSize;
      const int64_t lh = d[8];
      if (start == end && nn == 0 && lh < 0) {
        // the empty form: valid without leaves when nid is outside the root's range
        if (nl == 0) {
          uint32_t nid[8], rmn[8], rmx[8], rdg[8];
          load_ns29(nsp, nid);
          load_node90(a.roots + root_ix * kNodeSize, rmn, rmx, rdg);
          if (ns_less(nid, rmn) || ns_less(rmx, nid)) result = DAGPU_OK;
        }
        done = true;
      } else if (!done && lh >= 0) {
        // absence: nid < leafHash.min, read back from the proof's one leaf record
        uint32_t nid[8], hmn[8];
        load_ns29(nsp, nid);
        load_q(a.recs + rec0 * kRecNmt, hmn);
        if (!ns_less(nid, hmn)) done = true;
        nl = 1;  // the record stands for the one leaf of the fold
      }
    }
    if (done) end = 1;
  }
  int H = 0;
  while (H < kPvMaxHeight && ((int64_t)1 << H) < end) H++;
  int h = H, phase = kPvEval, csp = 0;
  int64_t lo = 0, next_leaf = 0, next_node = 0;
  int32_t ref = -1;
  bool okv = false, tail = false;
  long steps = 0;
  // visited subtrees <= 4 (nl + H) + 5, two steps each, then nn + 1 tail steps
  const long cap = 8 * (nl + H) + 2 * nn + 64;
  uint32_t vmn[8], vmx[8], vdg[8], lmn[8], lmx[8], ldg[8];
#pragma unroll
  for (int q = 0; q < 8; q++) vmn[q] = vmx[q] = vdg[q] = lmn[q] = lmx[q] = ldg[q] = 0;

  while (__any(!done)) {
    const bool wh = !done && phase == kPvHash;
    const bool step = !done && !wh;
    if (__any(step)) {
      if (step) {
        if (++steps > cap) {
          done = true;
        } else if (phase == kPvEval) {
          const int64_t hi = lo + ((int64_t)1 << h);
          if (h == 0 && start <= lo && lo < end) {
            if (next_leaf >= nl) {
              done = true;
            } else {
              const uint8_t* p = a.recs + (rec0 + next_leaf) * kRecNmt;
              load_q(p, vmn); load_q(p + 32, vmx); load_q(p + 64, vdg);
              next_leaf++;
              ref = -1; okv = true; phase = kPvAscend;
            }
          } else if (h == 0 || hi <= start || lo >= end) {
            if (next_node >= nn) {
              okv = false;
            } else {
              load_node90(a.nodes + (node_off + next_node) * kNodeSize, vmn, vmx, vdg);
              ref = (int32_t)next_node;
              next_node++;
              okv = true;
              if (pv_incomplete<NS>(nsp, hi <= start, vmn, vmx)) done = true;
            }
            phase = kPvAscend;
          } else {
            h--;
          }
        } else if (phase == kPvAscend) {
          if (h == H) {
            if (!okv) done = true; else phase = kPvTail;
          } else if (!((lo >> h) & 1)) {  // a left child is finished
            if (!okv) {
              h++;  // a missing left subtree fails its parent
            } else if (ref >= 0) {
              s_ref[h + 1][lane] = ref;
              lo += (int64_t)1 << h;
              phase = kPvEval;
            } else if (csp >= depth) {
              done = true;
            } else {
              uint8_t* p = a.cstack + (cs0 + csp) * kRecNmt;
              store_q(p, vmn); store_q(p + 32, vmx); store_q(p + 64, vdg);
              csp++;
              s_ref[h + 1][lane] = -1;
              lo += (int64_t)1 << h;
              phase = kPvEval;
            }
          } else {  // a right child is finished: fetch the parked left one
            lo -= (int64_t)1 << h;
            h++;
            const int32_t r = s_ref[h][lane];
            if (r >= 0) {
              load_node90(a.nodes + (node_off + r) * kNodeSize, lmn, lmx, ldg);
            } else if (csp > 0) {
              csp--;
              const uint8_t* p = a.cstack + (cs0 + csp) * kRecNmt;
              load_q(p, lmn); load_q(p + 32, lmx); load_q(p + 64, ldg);
            } else {
              done = true;
            }
            if (!okv) {  // a missing right subtree is skipped
#pragma unroll
              for (int q = 0; q < 8; q++) { vmn[q] = lmn[q]; vmx[q] = lmx[q]; vdg[q] = ldg[q]; }
              okv = true;
              ref = -1;
            } else {
              phase = kPvHash;
            }
          }
        } else {  // kPvTail: leftover nodes fold on the right, then the compare
          tail = true;
          if (next_node < nn) {
#pragma unroll
            for (int q = 0; q < 8; q++) { lmn[q] = vmn[q]; lmx[q] = vmx[q]; ldg[q] = vdg[q]; }
            load_node90(a.nodes + (node_off + next_node) * kNodeSize, vmn, vmx, vdg);
            next_node++;
            phase = kPvHash;
            if (pv_incomplete<NS>(nsp, false, vmn, vmx)) done = true;
          } else {
            uint32_t rmn[8], rmx[8], rdg[8];
            load_node90(a.roots + root_ix * kNodeSize, rmn, rmx, rdg);
            uint32_t diff = 0;
#pragma unroll
            for (int q = 0; q < 8; q++) {
              const uint32_t msk = q == 7 ? 0xFFu : 0xFFFFFFFFu;
              diff |= ((vmn[q] ^ rmn[q]) & msk) | ((vmx[q] ^ rmx[q]) & msk) | (vdg[q] ^ rdg[q]);
            }
            if (diff == 0 && next_leaf == nl) result = DAGPU_OK;
            done = true;
          }
        }
      }
    } else if (wh) {
      // nmt HashNode, IgnoreMaxNamespace: left (l*) and right (v*) -> v*
      if (ns_less(vmn, lmx)) {
        done = true;  // ErrUnorderedSiblings
      } else {
        auto get = [&](int P, int q) -> uint32_t {
          return P == 0 ? lmn[q] : P == 1 ? lmx[q] : P == 2 ? ldg[q] : P == 3 ? vmn[q] : P == 4 ? vmx[q] : vdg[q];
        };
        uint32_t st[8];
        sha_node_msg(get, st);
        const bool rpar = ns_is_parity(vmn);
#pragma unroll
        for (int q = 0; q < 8; q++) {
          if (rpar) vmx[q] = lmx[q];
          vmn[q] = lmn[q];
          vdg[q] = bswap32(st[q]);
        }
        ref = -1;
        okv = true;
        phase = tail ? kPvTail : kPvAscend;
      }
    }
  }
  if (i < a.n) a.status[i] = result;
}

// ---------------------------------------------------------------------------
// Merkle pass: one lane per crypto/merkle proof.  computeHashFromAunts descends
// from (index, total) taking the LAST aunt first; the lane records the side at
// each level on the way down (at most 63 levels: the total at least halves),
// then hashes from the leaf up with aunts[0], aunts[1], ...
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pv_merkle_kernel(PvMerkleArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const int64_t* d = a.desc + i * kPvDescMerkle;
  int64_t idx = d[0], tot = d[1];
  const int64_t na = d[2], aunt_off = d[3], leaf_ix = d[4], root_ix = d[5];
  int32_t result = DAGPU_ERR_PROOF;
  bool ok = !(tot < 0 || idx < 0) && !(idx >= tot || tot <= 0);
  uint64_t right = 0;  // bit lv: at depth lv from the top the path goes right
  int levels = 0;
  if (ok) {
#pragma unroll 1
    for (int it = 0; it < 64 && tot > 1; it++) {
      if (levels >= na) { ok = false; break; }
      const int64_t left = (int64_t)1 << (63 - __clzll(tot - 1));  // largest power of two below tot
      if (idx < left) {
        tot = left;
      } else {
        right |= (uint64_t)1 << levels;
        idx -= left;
        tot -= left;
      }
      levels++;
    }
    if (tot != 1 || levels != na) ok = false;  // aunts left over, or none left too early
  }
  uint32_t hsh[8];
  {
    uint32_t st[8];
    pv_sha_generic(nullptr, a.leaves + leaf_ix * a.leaf_len, a.leaf_len, st);
#pragma unroll
    for (int q = 0; q < 8; q++) hsh[q] = bswap32(st[q]);
  }
  if (a.leaf_hashes) {  // Proof.Verify: the proof's own LeafHash
    uint32_t lh[8];
    load_q(a.leaf_hashes + i * 32, lh);
    uint32_t diff = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) diff |= lh[q] ^ hsh[q];
    if (diff) ok = false;
  }
  if (ok) {
#pragma unroll 1
    for (int lv = levels - 1; lv >= 0; lv--) {
      uint32_t au[8], out[8];
      load_q(a.aunts + (aunt_off + (levels - 1 - lv)) * 32, au);
      if ((right >> lv) & 1) pv_rfc_inner(au, hsh, out); else pv_rfc_inner(hsh, au, out);
#pragma unroll
      for (int q = 0; q < 8; q++) hsh[q] = out[q];
    }
    uint32_t rt[8];
    load_q(a.roots + root_ix * 32, rt);
    uint32_t diff = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) diff |= rt[q] ^ hsh[q];
    if (diff == 0) result = DAGPU_OK;
  }
  a.status[i] = result;
}

hipError_t launch_pv_nmt_leaves(const PvNmtArgs& a, long n_records, hipStream_t s) {
  if (n_records <= 0) return hipSuccess;
  const dim3 grid((unsigned)((n_records + 255) / 256));
  if (a.namespace_rules)
    hipLaunchKernelGGL(pv_nmt_leaf_kernel<true>, grid, dim3(256), 0, s, a, n_records);
  else
    hipLaunchKernelGGL(pv_nmt_leaf_kernel<false>, grid, dim3(256), 0, s, a, n_records);
  return hipGetLastError();
}

hipError_t launch_pv_nmt_fold(const PvNmtArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  const dim3 grid((unsigned)((a.n + kPvFoldLanes - 1) / kPvFoldLanes));
  if (a.namespace_rules)
    hipLaunchKernelGGL(pv_nmt_fold_kernel<true>, grid, dim3(kPvFoldLanes), 0, s, a);
  else
    hipLaunchKernelGGL(pv_nmt_fold_kernel<false>, grid, dim3(kPvFoldLanes), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_pv_merkle(const PvMerkleArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(pv_merkle_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dagpu
