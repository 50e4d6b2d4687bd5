// proof_store.hip -- the batch proof store (dagpu_proof_store_device,
// include/dagpu.h): every node of every row tree and column tree of n extended
// squares resident in HBM, and each square's RFC-6962 tree over rowRoots ||
// colRoots up to the data root, built by a number of launches that does not
// depend on n.  What pkg/proof/proof.go:58-165 recomputes per query (the whole
// EDS, its trees and merkle.ProofsFromByteSlices) is kept once for the batch.
//
// Layout (share_proof_layout.hpp): three square-major regions.  The row and
// column slices of square i are byte for byte the stores of
// dagpu_row_nodes_device / dagpu_col_nodes_device (96-B records minNs[32] |
// maxNs[32] | digest[32], w = 2k):
//   row node (row, L, p)   record lvl(L) + row * (w >> L) + p,
//                          lvl(L) = sum_{l<L} w * (w >> l) = 2 w^2 - (w^2 >> (L - 1)), lvl(0) = 0
//   col node (col, L, p)   L >= 1: record lvl(L) - w^2 + col * (w >> L) + p; the
//                          leaf of column c at position p is row record p * w + c
//   DAH node (L, p)        digest dah_level_off(4k, L) + p, 32 B each
//
// Launches, each over ALL squares:
//   leaves      one lane per cell of the n (2k)^2 cells: the share-specialised
//               leaf hash of the square pipeline (share_leaf_sha256)
//   level L     L = 1 .. log2 w: one lane per output node, the row trees' and the
//               column trees' level L of every square in one grid (lanes ordered
//               square, axis, tree, node, so a wave stays inside one tree while
//               the level is at least a wave wide and the all-parity fast path
//               of the forest engine still applies per wave)
//   DAH level L L = 0 .. log2(4k): one lane per digest; level 0 hashes
//               0x00 | root90 from the two stores' top levels
// 1 + log2(2k) + log2(4k) + 1 launches: 19 at k = 128, for any n.
// No push-order check (the squares were extended; extend() reported it).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "forest.hpp"
#include "nmt_node.hpp"
#include "sha256.hpp"
#include "share_proof_layout.hpp"

namespace dagpu {

namespace {

__device__ __forceinline__ void ps_load8(const uint8_t* p, uint32_t (&d)[8]) {
  const uint4* q = (const uint4*)p;
  const uint4 x0 = q[0], x1 = q[1];
  d[0] = x0.x; d[1] = x0.y; d[2] = x0.z; d[3] = x0.w;
  d[4] = x1.x; d[5] = x1.y; d[6] = x1.z; d[7] = x1.w;
}

__device__ __forceinline__ void ps_store8(uint8_t* p, const uint32_t (&d)[8]) {
  uint4* q = (uint4*)p;
  q[0] = make_uint4(d[0], d[1], d[2], d[3]);
  q[1] = make_uint4(d[4], d[5], d[6], d[7]);
}

// first record of level L in a row store of w-leaf trees (ww = w * w)
__device__ __forceinline__ long ps_lvl(long ww, int L) { return L == 0 ? 0 : 2 * ww - (ww >> (L - 1)); }

// SHA-256 of a message of LEN bytes (56 <= LEN % 64 or LEN > 64: two blocks)
// held as little-endian dwords in memory byte order, zero beyond LEN
template <int LEN>
__device__ __forceinline__ void ps_sha_two_blocks(uint32_t (&m)[32], uint32_t (&out)[8]) {
  static_assert(LEN > 55 && LEN < 120, "two SHA-256 blocks");
  m[LEN >> 2] |= 0x80u << (8 * (LEN & 3));
  uint32_t st[8];
  sha256_init(st);
#pragma unroll
  for (int blk = 0; blk < 2; blk++) {
    uint32_t wv[16];
#pragma unroll
    for (int j = 0; j < 16; j++) wv[j] = bswap32(m[16 * blk + j]);
    if (blk == 1) { wv[14] = 0; wv[15] = (uint32_t)LEN * 8u; }
    sha256_compress(st, wv);
  }
#pragma unroll
  for (int j = 0; j < 8; j++) out[j] = bswap32(st[j]);
}

}  // namespace

// ---------------------------------------------------------------------------
// Leaves: lane = cell of square sq; the wrapper's namespace rule by cell
// coordinates (row < k and col < k: the share's own namespace, else parity).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void store_leaf_kernel(ProofStoreArgs a) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  const int logww = 2 * a.logw;
  const long sq = g >> logww;
  if (sq >= a.n) return;
  const long cell = g & ((1L << logww) - 1);
  const long r = cell >> a.logw, c = cell & (a.w - 1);
  const bool q0 = r < a.k && c < a.k;
  uint32_t st[8], ns[8];
  share_leaf_sha256((const uint4*)(a.eds + sq * a.square_stride + cell * kShareSize), q0, st, ns);
  if (!q0) {
#pragma unroll
    for (int j = 0; j < 7; j++) ns[j] = 0xFFFFFFFFu;
    ns[7] = 0xFFu;
  }
  uint4* o = (uint4*)(a.store + sq * a.row_bytes + cell * kRecNmt);
  o[0] = make_uint4(ns[0], ns[1], ns[2], ns[3]);
  o[1] = make_uint4(ns[4], ns[5], ns[6], ns[7]);
  o[2] = o[0];
  o[3] = o[1];
  o[4] = make_uint4(bswap32(st[0]), bswap32(st[1]), bswap32(st[2]), bswap32(st[3]));
  o[5] = make_uint4(bswap32(st[4]), bswap32(st[5]), bswap32(st[6]), bswap32(st[7]));
}

// ---------------------------------------------------------------------------
// Level L of every row tree and every column tree of every square: NMT
// HashNode with the IgnoreMaxNamespace rule, as forest_level_node.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void store_level_kernel(ProofStoreArgs a, int L) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  const int logper = a.logw - L;         // log2 of the nodes per tree at level L
  const int logaxis = a.logw + logper;   // ... per axis of one square
  const long sq = g >> (logaxis + 1);
  if (sq >= a.n) return;
  const int axis = (int)(g >> logaxis) & 1;
  const long t = (g >> logper) & (a.w - 1);
  const long j = g & ((1L << logper) - 1);
  const long w = a.w, ww = w * w, per = 1L << logper;
  const uint8_t* rows = a.store + sq * a.row_bytes;
  uint8_t* cols = a.store + a.col_off + sq * a.col_bytes;
  const uint8_t *lp, *rp;
  uint8_t* op;
  if (axis == 0) {
    lp = rows + (ps_lvl(ww, L - 1) + t * 2 * per + 2 * j) * kRecNmt;
    rp = lp + kRecNmt;
    op = a.store + sq * a.row_bytes + (ps_lvl(ww, L) + t * per + j) * kRecNmt;
  } else {
    if (L == 1) {  // the leaf of column t at position p is row record p * w + t
      lp = rows + (2 * j * w + t) * kRecNmt;
      rp = lp + w * kRecNmt;
    } else {
      lp = cols + (ps_lvl(ww, L - 1) - ww + t * 2 * per + 2 * j) * kRecNmt;
      rp = lp + kRecNmt;
    }
    op = cols + (ps_lvl(ww, L) - ww + t * per + j) * kRecNmt;
  }
  uint32_t lmn[8], lmx[8], ld[8], rmn[8], rmx[8], rd[8];
  ps_load8(lp, lmn); ps_load8(lp + 32, lmx); ps_load8(lp + 64, ld);
  ps_load8(rp, rmn); ps_load8(rp + 32, rmx); ps_load8(rp + 64, rd);
  uint32_t st[8];
  // waves whose children all carry the parity namespace (Q1..Q3) hash with
  // constant namespace words
  const bool lpar = ns_is_parity(lmn), rpar = ns_is_parity(rmn);
  if (__all(lpar && rpar)) {
    auto get = [&](int P, int i) -> uint32_t { return P == 2 ? ld[i] : P == 5 ? rd[i] : 0xFFFFFFFFu; };
    sha_node_msg<true, true, true>(get, st);
  } else if (__all(lpar)) {
    auto get = [&](int P, int i) -> uint32_t {
      return P <= 1 ? 0xFFFFFFFFu : P == 2 ? ld[i] : P == 3 ? rmn[i] : P == 4 ? rmx[i] : rd[i];
    };
    sha_node_msg<true>(get, st);
  } else {
    auto get = [&](int P, int i) -> uint32_t {
      return P == 0 ? lmn[i] : P == 1 ? lmx[i] : P == 2 ? ld[i] : P == 3 ? rmn[i] : P == 4 ? rmx[i] : rd[i];
    };
    sha_node_msg(get, st);
  }
  uint32_t dg[8];
#pragma unroll
  for (int i = 0; i < 8; i++) dg[i] = bswap32(st[i]);
  ps_store8(op, lmn);
  if (rpar) ps_store8(op + 32, lmx); else ps_store8(op + 32, rmx);  // IgnoreMaxNamespace
  ps_store8(op + 64, dg);
}

// ---------------------------------------------------------------------------
// DAH tree.  Level 0: leafHash(root90) = SHA256(0x00 | min(29) | max(29) |
// digest(32)) of the 4k axis roots; level L >= 1: SHA256(0x01 | l | r).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void store_dah_kernel(ProofStoreArgs a, int L) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  const int logn = a.logw + 1 - L;  // log2 of this level's digests per square
  const long sq = g >> logn;
  if (sq >= a.n) return;
  const long p = g & ((1L << logn) - 1);
  const long w = a.w, ww = w * w, leaves = 2 * w;
  uint8_t* dah = a.store + a.dah_off + sq * a.dah_bytes;
  uint32_t m[32], out[8];
#pragma unroll
  for (int j = 0; j < 32; j++) m[j] = 0;
  if (L == 0) {
    const long top = ps_lvl(ww, a.logw);  // the roots: the stores' top level
    const uint8_t* rec = p < w ? a.store + sq * a.row_bytes + (top + p) * kRecNmt
                               : a.store + a.col_off + sq * a.col_bytes + (top - ww + (p - w)) * kRecNmt;
    uint32_t mn[8], mx[8], dg[8];
    ps_load8(rec, mn); ps_load8(rec + 32, mx); ps_load8(rec + 64, dg);
    mn[7] &= 0xFFu;
    mx[7] &= 0xFFu;
    put_bytes<1>(m, mn);
    put_bytes<30>(m, mx);
    put_bytes<59>(m, dg);
    ps_sha_two_blocks<91>(m, out);
  } else {
    const uint8_t* in = dah + (dah_level_off(leaves, L - 1) + 2 * p) * kRecRfc;
    uint32_t l[8], r[8];
    ps_load8(in, l);
    ps_load8(in + kRecRfc, r);
    m[0] = 0x01u;
    put_bytes<1>(m, l);
    put_bytes<33>(m, r);
    ps_sha_two_blocks<65>(m, out);
  }
  ps_store8(dah + (dah_level_off(leaves, L) + p) * kRecRfc, out);
}

hipError_t launch_store_leaves(const ProofStoreArgs& a, hipStream_t s) {
  const long total = a.n * (long)a.w * a.w;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(store_leaf_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_store_level(const ProofStoreArgs& a, int L, hipStream_t s) {
  const long total = a.n * 2 * (long)a.w * (a.w >> L);
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(store_level_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, L);
  return hipGetLastError();
}

hipError_t launch_store_dah_level(const ProofStoreArgs& a, int L, hipStream_t s) {
  const long total = a.n * ((2L * a.w) >> L);
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(store_dah_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, L);
  return hipGetLastError();
}

}  // namespace dagpu
