// share_proof_layout.hpp -- layout of the batch proof store
// (dagpu_proof_store_device, proof_store.hip), request checks and output layout
// of the producer across squares (dagpu_nmt_prove_squares_device, nmt_prove.hip)
// and NewShareInclusionProof's row split (dagpu_share_proof_requests).  Host
// arithmetic only (no HIP include), so that tests/host/share_proof_layout_check.cpp
// can compile it without a GPU; the DAH-tree addressing the kernels share is
// marked for both sides when hipcc compiles it.
//
// Store of n squares of width k (w = 2k, 96-B NMT records, 32-B digests),
// square-major in each of three regions whose starts are 256-B aligned:
//   row store   at 0:       square i at i * row_bytes, the layout of
//               dagpu_row_nodes_device (levels 0 .. log2 w of every row tree)
//   col store   at col_off: square i at i * col_bytes, the layout of
//               dagpu_col_nodes_device (levels 1 .. log2 w of every column tree)
//   DAH tree    at dah_off: square i at i * (8k - 1) * 32: the RFC-6962 tree
//               over rowRoots || colRoots (4k leaves, a power of two: nothing is
//               promoted), level L after level L - 1, node (L, p) at digest
//               dah_level_off(4k, L) + p; the last digest is the data root.
//
// pkg/proof/proof.go:58-165 (NewShareInclusionProof) proves a range of ODS
// shares row by row under the row roots (lines 127-140) and every touched row
// root under the data root (merkle.ProofsFromByteSlices over rowRoots ||
// colRoots, lines 84-91): the aunts of leaf j are, leaf to root, the nodes
// (L, (j >> L) ^ 1) for L = 0 .. log2(4k) - 1.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "prove_layout.hpp"

namespace dagpu {

constexpr int kProveSqReqWords = 5;   // int64 per request: square, axis, index, start, end (DAGPU_PROVE_SQ_REQ_WORDS)
constexpr int kShareReqWords = 3;     // int64 per share range: square, start, end
constexpr int kMerkleDescWords = 6;   // int64 per merkle descriptor (DAGPU_MERKLE_DESC_WORDS)
constexpr size_t kStoreRec = 96, kStoreDigest = 32;

// first digest of level L of an RFC-6962 tree over `leaves` = 2^m leaves
DAGPU_PROVE_HD inline long dah_level_off(long leaves, int L) { return 2 * leaves - ((2 * leaves) >> L); }

// digest index of the aunt of leaf j at level L
DAGPU_PROVE_HD inline long dah_aunt_at(long leaves, long j, int L) { return dah_level_off(leaves, L) + ((j >> L) ^ 1); }

struct ProofStoreLayout {
  size_t row_bytes = 0, col_bytes = 0, dah_bytes = 0;  // per square
  size_t col_off = 0, dah_off = 0, total = 0;
};

// k a power of two, n >= 1 (the callers check); false when a size overflows
inline bool proof_store_layout(uint32_t k, size_t n, ProofStoreLayout* out) {
  const size_t w = 2 * (size_t)k;
  ProofStoreLayout l;
  l.row_bytes = w * (2 * w - 1) * kStoreRec;  // sum over levels of w * (w >> L)
  l.col_bytes = l.row_bytes - w * w * kStoreRec;
  l.dah_bytes = (4 * w - 1) * kStoreDigest;
  const size_t lim = ~(size_t)0 / 4;
  if (n == 0 || l.row_bytes > lim / n) return false;
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  l.col_off = up(n * l.row_bytes);
  l.dah_off = l.col_off + up(n * l.col_bytes);
  l.total = l.dah_off + up(n * l.dah_bytes);
  *out = l;
  return true;
}

// Why a batch was refused; kProveOk .. kProveSharesCap as prove_layout.
constexpr int kProveBadSquare = 16;  // square outside [0, n_sq)

// prove_layout for 5-word requests: the square is checked first, the other
// four words as the single-square call checks them (column nodes are always
// there).  On a refusal *bad is the first offending request (n for a capacity).
inline int prove_squares_layout(uint32_t k, size_t n_sq, size_t n, const int64_t* req, size_t nodes_cap,
                                bool check_shares, size_t shares_cap, ProveLayout* out, size_t* bad) {
  std::vector<int64_t> r4(n * kProveReqWords);
  for (size_t i = 0; i < n; i++) {
    const int64_t* r = req + i * kProveSqReqWords;
    for (int j = 0; j < kProveReqWords; j++) r4[i * kProveReqWords + j] = r[1 + j];
  }
  // the first offending request decides, whichever word is wrong: find the
  // first bad square, then let prove_layout look at the requests before it
  size_t first_sq = n;
  for (size_t i = 0; i < n; i++) {
    const int64_t sq = req[i * kProveSqReqWords];
    if (sq < 0 || (uint64_t)sq >= (uint64_t)n_sq) {
      first_sq = i;
      break;
    }
  }
  const ProveCheck pc = prove_layout(k, first_sq, r4.data(), true, ~(size_t)0, false, 0, out, bad);
  if (pc != kProveOk) return pc;
  if (first_sq < n) {
    *bad = first_sq;
    return kProveBadSquare;
  }
  if ((uint64_t)out->n_nodes > (uint64_t)nodes_cap) return kProveNodesCap;
  if (check_shares && (uint64_t)out->n_leaves > (uint64_t)shares_cap) return kProveSharesCap;
  return kProveOk;
}

// nmt descriptors of the produced proofs: as prove_fill_desc, but the roots
// table is the producer's own axis-root output (root_index = i).
inline void prove_squares_fill_desc(size_t n, const int64_t* req, const ProveLayout& lay, int64_t* desc) {
  for (size_t i = 0; i < n; i++) {
    const int64_t* r = req + i * kProveSqReqWords;
    int64_t* d = desc + i * kProveDescWords;
    d[0] = r[3];
    d[1] = r[4];
    d[2] = r[4] - r[3];
    d[3] = lay.leaf_off[i];
    d[4] = lay.node_off[i + 1] - lay.node_off[i];
    d[5] = lay.node_off[i];
    d[6] = (int64_t)i;
    d[7] = (int64_t)i;
  }
}

// dagpu_merkle_verify_batch descriptors of the axis roots under the data
// roots: { index, total, n_aunts, aunt_off, leaf_index, root_index }
inline void prove_squares_fill_mdesc(uint32_t k, size_t n, const int64_t* req, int64_t* mdesc) {
  const int64_t w = 2 * (int64_t)k;
  const int64_t la = prove_log2((uint32_t)(2 * w));
  for (size_t i = 0; i < n; i++) {
    const int64_t* r = req + i * kProveSqReqWords;
    int64_t* d = mdesc + i * kMerkleDescWords;
    d[0] = r[1] * w + r[2];
    d[1] = 2 * w;
    d[2] = la;
    d[3] = (int64_t)i * la;
    d[4] = (int64_t)i;
    d[5] = r[0];
  }
}

// One validated 5-word request as the kernels read it: two 8-B words, the
// four uint16 of prove_pack_req and the square.
inline void prove_squares_pack_req(const int64_t* r, int64_t* out2) {
  out2[0] = (int64_t)prove_pack_req(r + 1);
  out2[1] = r[0];
}

// NewShareInclusionProof's row split (pkg/proof/proof.go:63-67, 127-140): the
// range [start, end) of row-major ODS shares of one square, 0 <= start < end
// <= k^2, becomes one request per touched row: the first from start % k, the
// last to (end - 1) % k inclusive, the rows between whole [0, k); axis 0,
// index = the row.  span (n + 1) holds the prefix sums of rows per range.
// Nothing is written unless every range is valid and the rows fit `cap`.
inline bool share_proof_requests(uint32_t k, size_t n_sq, size_t n, const int64_t* sreq, int64_t* req_out,
                                 size_t cap, int64_t* span_out, size_t* n_req) {
  const int64_t kk = (int64_t)k * (int64_t)k;
  uint64_t rows = 0;
  for (size_t i = 0; i < n; i++) {
    const int64_t* s = sreq + i * kShareReqWords;
    if (s[0] < 0 || (uint64_t)s[0] >= (uint64_t)n_sq) return false;
    if (s[1] < 0 || s[1] >= s[2] || s[2] > kk) return false;
    rows += (uint64_t)((s[2] - 1) / k - s[1] / k + 1);
  }
  if (rows > (uint64_t)cap) return false;
  size_t at = 0;
  for (size_t i = 0; i < n; i++) {
    const int64_t* s = sreq + i * kShareReqWords;
    const int64_t start_row = s[1] / k, end_row = (s[2] - 1) / k;
    const int64_t start_leaf = s[1] % k, end_leaf = (s[2] - 1) % k;
    if (span_out) span_out[i] = (int64_t)at;
    for (int64_t row = start_row; row <= end_row; row++, at++) {
      int64_t* r = req_out + at * kProveSqReqWords;
      r[0] = s[0];
      r[1] = 0;
      r[2] = row;
      r[3] = row == start_row ? start_leaf : 0;
      r[4] = (row == end_row ? end_leaf : (int64_t)k - 1) + 1;
    }
  }
  if (span_out) span_out[n] = (int64_t)at;
  if (n_req) *n_req = at;
  return true;
}

}  // namespace dagpu
