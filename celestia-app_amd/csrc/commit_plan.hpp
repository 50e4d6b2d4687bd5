// commit_plan.hpp -- the commitment check laid out from the plans where they
// lie (dagpu_commit_plan_device / _host, dagpu_proposal_check_device) and the
// verdict of ProcessProposal's data-parallel part per block
// (dagpu_proposal_verdict_device / _host), in one copy for the host
// (commit_plan_host.cpp) and the device (commit_plan.hip).  Plain arithmetic
// only (no HIP include); every function is marked for both sides when hipcc
// compiles it.
//
// The layout is commit_layout.hpp's image (CommitLayout::words), built from the
// planner's arena and SpRecord[n] instead of host records:
//   blob[nblobs]{square, first_share} | share_pre[nblobs + 1] | sub_pre[nblobs + 1]
//   | sub[nsub]{blob, first leaf record, size} | work[nwork]
// Blocks go in order, each block's blobs in plan order.  A block contributes
// its blobs when its record has status 0, a plan (plan_bytes != 0) and the
// batch's width; every offset taken from the record or the plan header is
// bounded first (cp_block_blobs), and a block one of whose blobs has no share,
// or passes k * k, or whose blobs hold more than k * k shares together,
// contributes nothing: the sums below then stay inside the capacities a caller
// computes from (k, n) alone.
#pragma once
#include <stdint.h>

#include "blobtx_check.hpp"
#include "square_plan.hpp"

namespace dagpu {

// ---- inclusion.SubTreeWidth and MerkleMountainRangeSizes, without a vector ----
DAGPU_SQ_HD inline uint32_t cp_round_up_pow2(uint32_t v) {
  uint32_t r = 1;
  while (r < v) r <<= 1;
  return r;
}
DAGPU_SQ_HD inline uint32_t cp_log2(uint32_t pow2) {
  uint32_t l = 0;
  while ((1u << l) < pow2) l++;
  return l;
}
// min(RoundUpPowerOfTwo(ceil(count / threshold)), RoundUpPowerOfTwo(ceil(sqrt(count)))):
// the second is the least power of two p with p * p >= count.  count < 2^31.
DAGPU_SQ_HD inline uint32_t cp_subtree_width(uint32_t count, uint32_t threshold) {
  const uint32_t s = cp_round_up_pow2((uint32_t)(((uint64_t)count + threshold - 1) / threshold));
  uint32_t p = 1;
  while ((uint64_t)p * p < count) p <<= 1;
  return s < p ? s : p;
}
DAGPU_SQ_HD inline uint32_t cp_popcount(uint32_t v) {
  uint32_t n = 0;
  for (; v; v &= v - 1) n++;
  return n;
}
// The mountain range of `count` leaves under trees of w = 1 << lw leaves:
// count >> lw whole trees, then the set bits of the rest from high to low.
DAGPU_SQ_HD inline uint32_t cp_subtree_count(uint32_t count, uint32_t lw) {
  return (count >> lw) + cp_popcount(count & ((1u << lw) - 1));
}
// the subtrees of two leaves or more: they come before the one-leaf subtree
DAGPU_SQ_HD inline uint32_t cp_work_count(uint32_t count, uint32_t lw) {
  return (lw ? count >> lw : 0) + cp_popcount(count & ((1u << lw) - 1) & ~1u);
}
// subtree j < cp_subtree_count: its size; *first = its first leaf inside the blob
DAGPU_SQ_HD inline uint32_t cp_subtree(uint32_t count, uint32_t lw, uint32_t j, uint32_t* first) {
  const uint32_t full = count >> lw;
  if (j < full) {
    *first = j << lw;
    return 1u << lw;
  }
  uint32_t rest = count & ((1u << lw) - 1), top = 0;
  for (uint32_t i = full;; i++) {  // at most lw <= 10 steps
    top = 1;
    while ((top << 1) <= rest) top <<= 1;
    if (i == j) break;
    rest -= top;
  }
  *first = count - rest;
  return top;
}

// ---- a block's blobs ----------------------------------------------------------------
// The blob table of block `r`'s plan inside arena[0, cap), or nullptr (and
// *nblob = 0) when the block contributes nothing or the record or the header
// names a byte outside the plan or the arena.  Nothing outside is read.
DAGPU_SQ_HD inline const uint32_t* cp_block_blobs(const uint8_t* arena, uint64_t cap, const SpRecord& r, uint32_t k,
                                                  uint32_t* nblob) {
  *nblob = 0;
  if (r.status != 0 || r.plan_bytes == 0 || r.k != k) return nullptr;
  if (r.plan_bytes < sizeof(SqHdr) || (r.plan_off & 15) || r.plan_off > cap || r.plan_bytes > cap - r.plan_off)
    return nullptr;
  const SqHdr* h = (const SqHdr*)(arena + r.plan_off);
  const uint32_t nb = h->nblob, off = h->blob_off;
  if ((off & 3) || off > r.plan_bytes || (uint64_t)nb * kSqBlobWords * 4 > r.plan_bytes - off) return nullptr;
  if ((uint64_t)nb > (uint64_t)k * k) return nullptr;
  *nblob = nb;
  return (const uint32_t*)(arena + r.plan_off + off);
}

// What one blob adds to its block's sums; bad: the blob has no share or passes k * k
struct CpBlob {
  uint32_t shares, nsub, nwork, bad;
};
DAGPU_SQ_HD inline CpBlob cp_blob(const uint32_t* rec, uint32_t kk, uint32_t threshold) {
  const uint32_t first = rec[8], count = rec[9];
  CpBlob b;
  b.bad = count == 0 || first > kk || count > kk - first;
  if (b.bad) {
    b.shares = b.nsub = b.nwork = 0;
    return b;
  }
  const uint32_t lw = cp_log2(cp_subtree_width(count, threshold));
  b.shares = count;
  b.nsub = cp_subtree_count(count, lw);
  b.nwork = cp_work_count(count, lw);
  return b;
}

// per block, from the reduce pass; the scan turns them into the block's bases
struct CpSums {
  uint32_t nblobs, nshares, nsub, nwork, max_subtrees, pad[3];
};
DAGPU_SQ_HD inline CpSums cp_sums_zero() { return CpSums{0, 0, 0, 0, 0, {0, 0, 0}}; }
// a block whose blobs do not fit a square of the batch's width contributes nothing
DAGPU_SQ_HD inline CpSums cp_block_sums(uint32_t nblob, uint32_t shares, uint32_t nsub, uint32_t nwork,
                                        uint32_t max_subtrees, bool bad, uint32_t kk) {
  if (bad || shares > kk) return cp_sums_zero();
  return CpSums{nblob, shares, nsub, nwork, max_subtrees, {0, 0, 0}};
}

// the counts record: {nblobs, nshares, nsub, nwork, max_subtrees, 0, 0, 0}
constexpr uint32_t kCpCountWords = 8;
// word offsets of the tables inside the image, as CommitLayout's o_*
struct CpOffsets {
  uint64_t blob, share_pre, sub_pre, sub, work, words;
};
DAGPU_SQ_HD inline CpOffsets cp_offsets(uint32_t nblobs, uint32_t nsub, uint32_t nwork) {
  CpOffsets o;
  o.blob = 0;
  o.share_pre = 2 * (uint64_t)nblobs;
  o.sub_pre = o.share_pre + nblobs + 1;
  o.sub = o.sub_pre + nblobs + 1;
  o.work = o.sub + 3 * (uint64_t)nsub;
  o.words = o.work + nwork;
  return o;
}
// Capacities from (k, n) alone: n * k * k bounds the shares, rows, subtrees and
// blobs of a batch, half of it the work items (cp_block_sums).
DAGPU_SQ_HD inline uint64_t cp_cap_items(uint32_t k, uint64_t n) { return n * k * k; }
DAGPU_SQ_HD inline uint64_t cp_cap_table_words(uint32_t k, uint64_t n) {
  const uint64_t c = cp_cap_items(k, n);
  return 2 * c + 2 * (c + 1) + 3 * c + c / 2;
}

// One subtree record and its place in the work list: blob b (global index) of
// `count` shares whose leaf records start at share0, subtrees at sub0, work
// items at work0; j the subtree inside the blob.
DAGPU_SQ_HD inline void cp_put_subtree(uint32_t* tables, const CpOffsets& o, uint32_t b, uint32_t count, uint32_t lw,
                                       uint32_t share0, uint32_t sub0, uint32_t work0, uint32_t j) {
  uint32_t first;
  const uint32_t size = cp_subtree(count, lw, j, &first);
  uint32_t* q = tables + o.sub + 3 * (uint64_t)(sub0 + j);
  q[0] = b;
  q[1] = share0 + first;
  q[2] = size;
  if (size >= 2) tables[o.work + work0 + j] = sub0 + j;
}

// what the three layout passes read and write
struct CpArgs {
  const uint8_t* arena;
  uint64_t arena_cap;
  const SpRecord* rec;
  uint32_t n, k, threshold;
  CpSums* sums;         // n: each block's sums (reduce)
  CpSums* base;         // n: the sums of the blocks before it (scan)
  uint32_t* tables;     // the image, cp_cap_table_words(k, n) words
  uint32_t* counts;     // kCpCountWords
  uint64_t* blob_base;  // n + 1
};

// The three passes as host loops (dagpu_commit_plan_host): the same per-blob and
// per-subtree functions, one block and one blob after the other.
inline void cp_layout_host(const CpArgs& a) {
  const uint32_t kk = a.k * a.k;
  for (uint32_t blk = 0; blk < a.n; blk++) {
    uint32_t nblob;
    const uint32_t* blobs = cp_block_blobs(a.arena, a.arena_cap, a.rec[blk], a.k, &nblob);
    uint64_t shares = 0;
    uint32_t nsub = 0, nwork = 0, mx = 0;
    bool bad = false;
    for (uint32_t i = 0; i < nblob && !bad; i++) {
      const CpBlob b = cp_blob(blobs + (uint64_t)i * kSqBlobWords, kk, a.threshold);
      shares += b.shares;
      nsub += b.nsub;
      nwork += b.nwork;
      mx = b.nsub > mx ? b.nsub : mx;
      bad = b.bad || shares > kk;
    }
    a.sums[blk] = cp_block_sums(nblob, (uint32_t)(bad ? 0 : shares), nsub, nwork, mx, bad, kk);
  }
  CpSums at = cp_sums_zero();
  for (uint32_t blk = 0; blk < a.n; blk++) {
    const CpSums s = a.sums[blk];
    a.base[blk] = at;
    a.base[blk].max_subtrees = 0;
    a.blob_base[blk] = at.nblobs;
    at.nblobs += s.nblobs;
    at.nshares += s.nshares;
    at.nsub += s.nsub;
    at.nwork += s.nwork;
    at.max_subtrees = s.max_subtrees > at.max_subtrees ? s.max_subtrees : at.max_subtrees;
  }
  for (uint32_t j = 0; j < kCpCountWords; j++) a.counts[j] = 0;
  a.counts[0] = at.nblobs;
  a.counts[1] = at.nshares;
  a.counts[2] = at.nsub;
  a.counts[3] = at.nwork;
  a.counts[4] = at.max_subtrees;
  a.blob_base[a.n] = at.nblobs;
  const CpOffsets o = cp_offsets(at.nblobs, at.nsub, at.nwork);
  a.tables[o.share_pre + at.nblobs] = at.nshares;
  a.tables[o.sub_pre + at.nblobs] = at.nsub;
  for (uint32_t blk = 0; blk < a.n; blk++) {
    if (a.sums[blk].nblobs == 0) continue;
    uint32_t nblob;
    const uint32_t* blobs = cp_block_blobs(a.arena, a.arena_cap, a.rec[blk], a.k, &nblob);
    const CpSums base = a.base[blk];
    uint32_t share0 = base.nshares, sub0 = base.nsub, work0 = base.nwork;
    for (uint32_t i = 0; i < nblob; i++) {
      const uint32_t* rec = blobs + (uint64_t)i * kSqBlobWords;
      const uint32_t count = rec[9], lw = cp_log2(cp_subtree_width(count, a.threshold));
      const uint64_t g = (uint64_t)base.nblobs + i;
      a.tables[o.blob + 2 * g] = blk;
      a.tables[o.blob + 2 * g + 1] = rec[8];
      a.tables[o.share_pre + g] = share0;
      a.tables[o.sub_pre + g] = sub0;
      const uint32_t t = cp_subtree_count(count, lw);
      for (uint32_t j = 0; j < t; j++) cp_put_subtree(a.tables, o, (uint32_t)g, count, lw, share0, sub0, work0, j);
      share0 += count;
      sub0 += t;
      work0 += cp_work_count(count, lw);
    }
  }
}

// ---- the verdict --------------------------------------------------------------------
enum : uint32_t {
  kPvAccept = 0,
  kPvNonBlobTxHasPfb = 1,
  kPvInvalidBlobTx = 2,
  kPvCalculateCommitment = 3,
  kPvInvalidShareCommitment = 4,
  kPvConstructFailed = 5,
  kPvSquareSizeDiffers = 6,
  kPvNotJudged = 7,
  kPvExtendFailed = 8,
  kPvDataRootDiffers = 9,
};
constexpr uint32_t kPvNone = 0xFFFFFFFFu;
constexpr uint64_t kPvNoKey = ~(uint64_t)0;
constexpr uint32_t kPvCommitMismatch = 1, kPvCommitPushOrder = 2;  // DAGPU_COMMIT_*

// The key of a row whose commitment failed: ValidateBlobTx (blob_tx.go:91-100)
// walks a tx's blobs in order, computes blob i's commitment (the push-order
// fault) and then compares it, so the lowest (tx, blob, push order before
// mismatch) is the failure the reference reports.  A row tied to no tx keeps
// tx = kPvNone: it orders after every tx and still rejects the block.
DAGPU_SQ_HD inline uint64_t pv_commit_key(uint32_t tx, uint32_t blob_in_tx, uint32_t commit_status) {
  const uint32_t b = blob_in_tx > 0x7FFFFFFEu ? 0x7FFFFFFEu : blob_in_tx;
  return (uint64_t)tx << 32 | (uint64_t)b << 1 | (commit_status & kPvCommitPushOrder ? 0 : 1);
}

struct PvIn {
  uint32_t plan_status, block_k, k;  // the record's status and width, the batch's width
  uint32_t st_tx, st_word;           // d_block_status: the lowest stateless failure, or kPvNone
  uint64_t commit_key;               // the lowest pv_commit_key of the block's rows, or kPvNoKey
  uint32_t have_size, size;          // the proposed square size
  uint32_t extend_status;
  uint32_t root_differs;             // data hashes were given and the 32 bytes differ
};
struct PvOut {
  uint32_t code, tx, word, aux;
};
// ProcessProposal's order (app/process_proposal.go): the tx loop (:53-132) with
// the commitment comparison inside ValidateBlobTx (:120), a stateless failure
// before a commitment failure of the same tx; then square.Construct (:135), the
// square size (:142), extend (:147) and the data root (:161).
DAGPU_SQ_HD inline PvOut pv_block(const PvIn& v) {
  PvOut o{kPvAccept, kPvNone, 0, 0};
  const bool have_st = v.st_tx != kPvNone, have_c = v.commit_key != kPvNoKey;
  const uint32_t c_tx = (uint32_t)(v.commit_key >> 32);
  if (have_st && (!have_c || v.st_tx <= c_tx)) {
    o.code = (v.st_word & 0xFF) == kBtNonBlobTxHasPfb ? kPvNonBlobTxHasPfb : kPvInvalidBlobTx;
    o.tx = v.st_tx;
    o.word = v.st_word;
  } else if (have_c) {
    o.code = (v.commit_key & 1) ? kPvInvalidShareCommitment : kPvCalculateCommitment;
    o.tx = c_tx;
    o.aux = (uint32_t)(v.commit_key & 0xFFFFFFFFu) >> 1;
  } else if (v.plan_status) {
    o.code = kPvConstructFailed;
    o.word = v.plan_status;
  } else if (v.have_size && v.size != v.block_k) {
    o.code = kPvSquareSizeDiffers;
    o.aux = v.block_k;
  } else if (v.block_k != v.k) {
    o.code = kPvNotJudged;
  } else if (v.extend_status) {
    o.code = kPvExtendFailed;
  } else if (v.root_differs) {
    o.code = kPvDataRootDiffers;
  }
  return o;
}

// The block that owns row `row`: the last block with blob_base <= row (n >= 1)
DAGPU_SQ_HD inline uint32_t pv_row_block(const uint64_t* blob_base, uint32_t n, uint64_t row) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (blob_base[mid] <= row) lo = mid;
    else hi = mid;
  }
  return lo;
}

// what the two verdict passes read and write
struct PvArgs {
  const SpRecord* rec;
  const uint32_t* block_status;  // n x {tx, word}
  const int32_t* blob_status;    // per row
  const uint32_t* row_tx;        // per row {tx, blob index in the tx}
  const uint64_t* blob_base;     // n + 1
  const int32_t* extend_status;  // n, or null
  const uint8_t* dah;            // n x 32, or null
  const uint8_t* hashes;         // n x 32, or null
  const uint32_t* sizes;         // n, or null
  unsigned long long* key;       // n, kPvNoKey before the fold
  uint32_t* verdicts;            // n x 4
  uint32_t n, k;
};
// row -> its key and block; false: the row's commitment is in order
DAGPU_SQ_HD inline bool pv_row_key(const PvArgs& a, uint64_t row, uint32_t* blk, uint64_t* key) {
  const uint32_t st = (uint32_t)a.blob_status[row];
  if (!st) return false;
  *blk = pv_row_block(a.blob_base, a.n, row);
  *key = pv_commit_key(a.row_tx[2 * row], a.row_tx[2 * row + 1], st);
  return true;
}
DAGPU_SQ_HD inline void pv_finish_block(const PvArgs& a, uint32_t i) {
  const SpRecord r = a.rec[i];
  PvIn v;
  v.plan_status = r.status;
  v.block_k = r.k;
  v.k = a.k;
  v.st_tx = a.block_status[2 * i];
  v.st_word = a.block_status[2 * i + 1];
  v.commit_key = a.key[i];
  v.have_size = a.sizes != nullptr;
  v.size = a.sizes ? a.sizes[i] : 0;
  v.extend_status = a.extend_status ? (uint32_t)a.extend_status[i] : 0;
  v.root_differs = 0;
  if (a.hashes && a.dah)
    for (uint32_t q = 0; q < 32; q++) v.root_differs |= a.hashes[32 * (uint64_t)i + q] != a.dah[32 * (uint64_t)i + q];
  const PvOut o = pv_block(v);
  uint32_t* out = a.verdicts + 4 * (uint64_t)i;
  out[0] = o.code;
  out[1] = o.tx;
  out[2] = o.word;
  out[3] = o.aux;
}

// the two verdict passes as host loops (dagpu_proposal_verdict_host); key[] holds kPvNoKey
inline void pv_host(const PvArgs& a) {
  const uint64_t rows = a.blob_base[a.n];
  for (uint64_t row = 0; row < rows; row++) {
    uint32_t blk;
    uint64_t key;
    if (pv_row_key(a, row, &blk, &key) && key < a.key[blk]) a.key[blk] = key;
  }
  for (uint32_t i = 0; i < a.n; i++) pv_finish_block(a, i);
}

}  // namespace dagpu
