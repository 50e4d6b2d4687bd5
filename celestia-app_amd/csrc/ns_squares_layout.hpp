// ns_squares_layout.hpp -- host arithmetic of the namespace producer across the
// squares of a batch proof store (dagpu_nmt_namespace_squares_count_device,
// dagpu_nmt_prove_namespace_squares_device; kernels in nmt_namespace.hip): the
// workspace carve, the packed range word of a (query, square, row), the hit
// record a proof sends to the host, the re-check of those records, the
// capacity check and the descriptor fill.  Plain arithmetic only (no HIP
// include), so that tests/host/ns_squares_layout_check.cpp can compile it
// without a GPU; the word's pack / unpack and the four summed quantities are
// marked for both sides when hipcc compiles it.
//
// Lanes: one per (query, square, row), t = (query * n_sq + square) * 2k + row,
// so ascending t is the (query, square, row) order of the proofs.  Blocks of
// kNsSqBlock lanes; the exclusive prefix sum over all lanes of the four
// quantities { proofs, absence proofs, proof nodes, proven cells } is done in
// three steps: per-block sums, a scan of the block sums in chunks of
// kNsSqBlock with per-chunk sums (level 1) and a scan of the chunk sums by one
// workgroup that loops (level 2), so lane t starts at
//   bsum[t / 256] + csum[t / 65536] + (prefix inside its block).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "prove_layout.hpp"
#include "share_proof_layout.hpp"

namespace dagpu {

constexpr int kNsHitWords = 6;     // int32 per proof on the host: query, square, row, kind, start, end (DAGPU_NS_HIT_WORDS)
constexpr int kNsHitRecWords = 2;  // uint32 per proof from the device: lane, range word
constexpr int kNsNmtDescWords = 9; // int64 per nmt descriptor (DAGPU_NMT_NS_DESC_WORDS)
constexpr int kNsSqBlock = 256;    // lanes per block, and block sums per chunk
constexpr int kNsSqSums = 4;       // proofs, absence proofs, proof nodes, proven cells
constexpr uint64_t kNsSqMaxLanes = ((uint64_t)1 << 31) - kNsSqBlock;  // lanes and hit records index with 32 bits

// The range of one lane in 32 bits: kind in bits 0-1, start in bits 2-16 and
// end - start - 1 in bits 17-31; 0 when outside.  A hit has 0 <= start < end
// <= w <= 32768, so start and end - start - 1 are both below 2^15.
DAGPU_PROVE_HD inline uint32_t ns_sq_pack(int kind, uint32_t start, uint32_t end) {
  if (kind == 0) return 0;
  return (uint32_t)kind | (start << 2) | ((end - start - 1) << 17);
}

DAGPU_PROVE_HD inline void ns_sq_unpack(uint32_t v, int* kind, uint32_t* start, uint32_t* end) {
  *kind = (int)(v & 3u);
  if (*kind == 0) {
    *start = *end = 0;
    return;
  }
  *start = (v >> 2) & 0x7FFFu;
  *end = *start + (v >> 17) + 1;
}

// what a lane adds to the four sums (m = log2 of the leaves per tree)
DAGPU_PROVE_HD inline void ns_sq_quantities(uint32_t v, int m, int64_t q[kNsSqSums]) {
  int kind;
  uint32_t s, e;
  ns_sq_unpack(v, &kind, &s, &e);
  q[0] = kind != 0;
  q[1] = kind == 2;
  q[2] = kind != 0 ? prove_node_count(m, s, e) : 0;
  q[3] = kind == 1 ? (int64_t)(e - s) : 0;
}

// Byte offsets into the workspace, each 256-B aligned.  The dense part is
// 4 B per lane (the words); everything else is per query, per block, per
// (query, square) or per proof of proofs_cap.
struct NsSqCarve {
  uint64_t lanes = 0, pairs = 0, blocks = 0, chunks = 0;  // (q, sq, row); (q, sq); blocks of lanes; chunks of blocks
  size_t queries = 0;   // n_q x 32 B, zero padded
  size_t words = 0;     // lanes x uint32
  size_t bsum = 0;      // blocks x 4 int64: block sums, then their exclusive scan inside each chunk
  size_t csum = 0;      // chunks x 4 int64: chunk sums, then their exclusive scan
  size_t totals = 0;    // 4 int64
  size_t per = 0;       // pairs x int32: proofs per (query, square)
  size_t req = 0;       // proofs_cap x { prove_pack_req word, square } int64
  size_t node_off = 0;  // proofs_cap + 1 int64
  size_t leaf_off = 0;  // proofs_cap + 1 int64
  size_t abs_rec = 0;   // proofs_cap int64: level-0 record of each absence proof in the row region
  size_t hits = 0;      // proofs_cap x kNsHitRecWords uint32
  size_t total = 0;
};

// k a power of two <= 16384; false when n_sq = 0 or a count or size overflows
inline bool ns_squares_carve(uint32_t k, size_t n_sq, size_t n_q, size_t proofs_cap, NsSqCarve* out) {
  const uint64_t w = 2 * (uint64_t)k;
  NsSqCarve c;
  if (n_sq == 0 || w == 0 || w > 32768) return false;
  if (n_q > kNsSqMaxLanes / w || (uint64_t)n_q * w > kNsSqMaxLanes / n_sq) return false;
  if ((uint64_t)proofs_cap > ((uint64_t)1 << 40)) return false;
  c.pairs = (uint64_t)n_q * n_sq;
  c.lanes = c.pairs * w;
  c.blocks = (c.lanes + kNsSqBlock - 1) / kNsSqBlock;
  c.chunks = (c.blocks + kNsSqBlock - 1) / kNsSqBlock;
  size_t at = 0;
  auto take = [&at](uint64_t bytes) {
    const size_t here = at;
    at += (size_t)((bytes + 255) & ~(uint64_t)255);
    return here;
  };
  c.queries = take(32 * (uint64_t)n_q);
  c.words = take(4 * c.lanes);
  c.bsum = take(c.blocks * kNsSqSums * 8);
  c.csum = take(c.chunks * kNsSqSums * 8);
  c.totals = take(kNsSqSums * 8);
  c.per = take(c.pairs * 4);
  c.req = take((uint64_t)proofs_cap * 16);
  c.node_off = take(((uint64_t)proofs_cap + 1) * 8);
  c.leaf_off = take(((uint64_t)proofs_cap + 1) * 8);
  c.abs_rec = take((uint64_t)proofs_cap * 8);
  c.hits = take((uint64_t)proofs_cap * kNsHitRecWords * 4);
  c.total = at + 256;
  *out = c;
  return true;
}

// The most nodes one proof can have in a tree of 2^m leaves: popcount(start) +
// m - popcount(end - 1) is largest for the two leaves astride the middle,
// [2^(m-1) - 1, 2^(m-1) + 1): (m - 1) + m - 1.  A tree of two leaves has at
// most one.
inline int ns_sq_max_nodes(int m) { return m <= 1 ? m : 2 * m - 2; }

// The four totals the device reports, before anything is sized from them:
// every proof is one lane, has at most ns_sq_max_nodes(m) nodes (an absence
// proof, one leaf wide, exactly m) and at most w cells.
inline bool ns_sq_totals_ok(const int64_t t[kNsSqSums], uint64_t lanes, int m, uint32_t w) {
  if (t[0] < 0 || (uint64_t)t[0] > lanes) return false;
  if (t[1] < 0 || t[1] > t[0]) return false;
  if (t[2] < t[1] * m || t[2] > t[1] * m + (t[0] - t[1]) * ns_sq_max_nodes(m)) return false;
  if (t[3] < 0 || t[3] > (t[0] - t[1]) * (int64_t)w) return false;
  return true;
}

// Which capacity is too small for the need { proofs, absence proofs, nodes,
// cells }: 0 .. 3 in that order, -1 when all four fit.
inline int ns_sq_short_capacity(const int64_t need[kNsSqSums], size_t proofs_cap, size_t leaf_hashes_cap,
                                size_t nodes_cap, size_t shares_cap) {
  if ((uint64_t)need[0] > (uint64_t)proofs_cap) return 0;
  if ((uint64_t)need[1] > (uint64_t)leaf_hashes_cap) return 1;
  if ((uint64_t)need[2] > (uint64_t)nodes_cap) return 2;
  if ((uint64_t)need[3] > (uint64_t)shares_cap) return 3;
  return -1;
}

// One device hit record as the six host words.  The lane is split whatever it
// holds: ns_sq_hit_ok judges the result.
inline void ns_sq_unpack_hit(const uint32_t rec[kNsHitRecWords], size_t n_sq, uint32_t w, int32_t h[kNsHitWords]) {
  const uint64_t lane = rec[0], pair = lane / w;
  int kind;
  uint32_t s, e;
  ns_sq_unpack(rec[1], &kind, &s, &e);
  h[0] = (int32_t)(pair / n_sq);
  h[1] = (int32_t)(pair % n_sq);
  h[2] = (int32_t)(lane % w);
  h[3] = kind;
  h[4] = (int32_t)s;
  h[5] = (int32_t)e;
}

// The re-check of one hit: query, square and row in range, kind present or
// absent, 0 <= start < end <= w, and an absence proof is one leaf wide.
inline bool ns_sq_hit_ok(const int32_t h[kNsHitWords], size_t n_q, size_t n_sq, uint32_t w) {
  if (h[0] < 0 || (uint64_t)h[0] >= (uint64_t)n_q) return false;
  if (h[1] < 0 || (uint64_t)h[1] >= (uint64_t)n_sq) return false;
  if (h[2] < 0 || (uint32_t)h[2] >= w) return false;
  if (h[3] != 1 && h[3] != 2) return false;
  if (!(0 <= h[4] && h[4] < h[5] && (uint32_t)h[5] <= w)) return false;
  if (h[3] == 2 && h[5] - h[4] != 1) return false;
  return true;
}

// Re-check n device hit records against the totals they were laid out by and
// write them as host words: every record passes ns_sq_hit_ok, the lanes ascend
// strictly (the order is part of the contract) and the four sums over the
// records are the totals.  False on the first violation; `hits` then holds
// nothing to use.
inline bool ns_sq_check_hits(size_t n, const uint32_t* rec, size_t n_q, size_t n_sq, uint32_t w,
                             const int64_t totals[kNsSqSums], int32_t* hits) {
  const int m = prove_log2(w);
  const uint64_t lanes = (uint64_t)n_q * n_sq * w;
  int64_t sum[kNsSqSums] = {0, 0, 0, 0};
  for (size_t i = 0; i < n; i++) {
    const uint32_t* r = rec + i * kNsHitRecWords;
    if (r[0] >= lanes || (i && r[0] <= rec[(i - 1) * kNsHitRecWords])) return false;
    int32_t* h = hits + i * kNsHitWords;
    ns_sq_unpack_hit(r, n_sq, w, h);
    if (!ns_sq_hit_ok(h, n_q, n_sq, w)) return false;
    int64_t q[kNsSqSums];
    ns_sq_quantities(r[1], m, q);
    for (int j = 0; j < kNsSqSums; j++) sum[j] += q[j];
  }
  for (int j = 0; j < kNsSqSums; j++)
    if (sum[j] != totals[j]) return false;
  return true;
}

// Descriptors of n checked hits in order.  desc (9 words per proof, may be
// null): { start, end, n_leaves, leaf_off, n_nodes, node_off, ns_index = query,
// root_index = i, leaf_hash_index } with n_leaves = 0 and leaf_hash_index = the
// running absence count for an absence proof, -1 otherwise; the offsets are
// the running sums the device scan gives the same proofs.  mdesc (6 words, may
// be null): { row, 4k, log2(4k), i * log2(4k), i, square }.
inline void ns_sq_fill_desc(uint32_t k, size_t n, const int32_t* hits, int64_t* desc, int64_t* mdesc) {
  const int64_t w = 2 * (int64_t)k;
  const int m = prove_log2((uint32_t)w);
  const int64_t la = m + 1;
  int64_t nodes = 0, cells = 0, n_abs = 0;
  for (size_t i = 0; i < n; i++) {
    const int32_t* h = hits + i * kNsHitWords;
    const bool absent = h[3] == 2;
    const int64_t nn = prove_node_count(m, (uint32_t)h[4], (uint32_t)h[5]);
    const int64_t nl = absent ? 0 : h[5] - h[4];
    if (desc) {
      int64_t* d = desc + i * kNsNmtDescWords;
      d[0] = h[4];
      d[1] = h[5];
      d[2] = nl;
      d[3] = cells;
      d[4] = nn;
      d[5] = nodes;
      d[6] = h[0];
      d[7] = (int64_t)i;
      d[8] = absent ? n_abs : -1;
    }
    if (mdesc) {
      int64_t* d = mdesc + i * kMerkleDescWords;
      d[0] = h[2];
      d[1] = 2 * w;
      d[2] = la;
      d[3] = (int64_t)i * la;
      d[4] = (int64_t)i;
      d[5] = h[1];
    }
    nodes += nn;
    cells += nl;
    n_abs += absent;
  }
}

}  // namespace dagpu
