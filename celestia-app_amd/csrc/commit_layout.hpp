// commit_layout.hpp -- request checks and device tables of the share
// commitments computed from squares resident in HBM
// (dagpu_blob_commitments_device, blob_commit.hip).  Host arithmetic only (no
// HIP include), so that tests/host/commit_layout_check.cpp can compile it
// without a GPU.
//
// inclusion.CreateCommitment (pkg/inclusion/commitment.go:19-75) of a blob of
// `count` shares: w = SubTreeWidth(count, threshold)
// (blob_share_commitment_rules.go:85-101), the shares cut into the subtrees of
// MerkleMountainRangeSizes(count, w) (commitment.go:85-107), one nmt root per
// subtree, then merkle.HashFromByteSlices over the roots.
//
// The kernels check nothing: every index they form comes from the tables laid
// out here, and commit_layout refuses whatever would not fit them.
//
// Device image (uint32 words, CommitLayout::words):
//   blob[nblobs]        {square, first_share}
//   share_pre[nblobs+1] prefix sums of share counts: blob b's leaf records are
//                       [share_pre[b], share_pre[b+1])
//   sub_pre[nblobs+1]   prefix sums of subtree counts
//   sub[nsub]           {blob, first leaf record, size}, subtree-major: the
//                       subtrees of a blob cover its leaf records once, in order
//   work[nwork]         indexes of the subtrees of size >= 2 (the ones to reduce)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace dagpu {

constexpr int kCommitReqWords = 3;         // int64 per blob: square, first_share, share_count
constexpr uint32_t kCommitMaxWidth = 1024;  // the plan format's kSqMaxWidth
constexpr int kCommitBlobWords = 2, kCommitSubWords = 3;

inline uint64_t commit_round_up_pow2(uint64_t v) {
  uint64_t r = 1;
  while (r < v) r <<= 1;
  return r;
}

// inclusion.SubTreeWidth: min(RoundUpPowerOfTwo(ceil(count / threshold)),
// RoundUpPowerOfTwo(ceil(sqrt(count)))), in integers
inline uint64_t commit_subtree_width(uint64_t count, uint64_t threshold) {
  const uint64_t s = commit_round_up_pow2((count + threshold - 1) / threshold);
  uint64_t r = 0;  // ceil(sqrt(count))
  while (r * r < count) r++;
  const uint64_t min_sq = commit_round_up_pow2(r);
  return s < min_sq ? s : min_sq;
}

// inclusion.MerkleMountainRangeSizes: trees of max_tree leaves while they fit,
// then the set bits of the rest from high to low.  Appends to `out`, returns
// how many it appended.
inline size_t commit_mountain_sizes(uint64_t total, uint64_t max_tree, std::vector<uint32_t>* out) {
  size_t n = 0;
  while (total != 0) {
    uint64_t t = max_tree;
    if (total < max_tree) {
      const uint64_t up = commit_round_up_pow2(total);
      t = up == total ? up : up / 2;
    }
    out->push_back((uint32_t)t);
    total -= t;
    n++;
  }
  return n;
}

// Why a call was refused (commit_layout); kCommitOk otherwise.
enum CommitCheck {
  kCommitOk = 0,
  kCommitBadWidth,      // k not a power of two
  kCommitWideSquare,    // k > 1024 (DAGPU_ERR_UNSUPPORTED)
  kCommitBadThreshold,  // threshold == 0
  kCommitBadPitch,      // row_pitch < k * 512
  kCommitMisaligned,    // base, square_stride or row_pitch not a multiple of 16
  kCommitBadSquare,     // a record's square outside [0, n)
  kCommitBadCount,      // a record's share_count < 1
  kCommitBadRange,      // first_share < 0 or first_share + share_count > k * k
  kCommitTooMany,       // 2^31 shares or more in one call
};

inline const char* commit_check_text(CommitCheck c) {
  static const char* const why[] = {"",
                                    "square width must be a power of two",
                                    "square width above 1024 is not supported",
                                    "subtree root threshold must be positive",
                                    "row_pitch below k * 512",
                                    "d_squares, square_stride and row_pitch must be multiples of 16",
                                    "square index outside [0, n)",
                                    "share_count below 1",
                                    "range is not 0 <= first_share, first_share + share_count <= k * k",
                                    "2^31 shares or more in one call"};
  return why[c];
}

struct CommitLayout {
  std::vector<uint32_t> words;  // the device image, see above
  size_t nblobs = 0, nshares = 0, nsub = 0, nwork = 0;
  uint32_t max_subtrees = 0;  // the most subtrees of one blob
  // word offsets of the tables inside `words`
  size_t o_blob = 0, o_share_pre = 0, o_sub_pre = 0, o_sub = 0, o_work = 0;
};

// Check the call's geometry and every record, then lay the tables out.  On a
// refusal *bad is the first offending blob (nblobs where the refusal is not a
// blob's) and `out` holds nothing to use.
inline CommitCheck commit_layout(uint32_t k, size_t n, size_t nblobs, const int64_t* blobs, uint64_t base_addr,
                                 size_t square_stride, size_t row_pitch, uint32_t threshold, CommitLayout* out,
                                 size_t* bad) {
  *bad = nblobs;
  if (k == 0 || (k & (k - 1)) != 0) return kCommitBadWidth;
  if (k > kCommitMaxWidth) return kCommitWideSquare;
  if (threshold == 0) return kCommitBadThreshold;
  if (row_pitch < (size_t)k * 512) return kCommitBadPitch;
  if ((base_addr | square_stride | row_pitch) & 15) return kCommitMisaligned;
  const int64_t kk = (int64_t)k * k;
  uint64_t nshares = 0;
  for (size_t b = 0; b < nblobs; b++) {
    const int64_t* r = blobs + b * kCommitReqWords;
    *bad = b;
    if (r[0] < 0 || (uint64_t)r[0] >= (uint64_t)n) return kCommitBadSquare;
    if (r[2] < 1) return kCommitBadCount;
    if (r[1] < 0 || r[1] > kk || r[2] > kk - r[1]) return kCommitBadRange;
    nshares += (uint64_t)r[2];
    if (nshares >= ((uint64_t)1 << 31)) return kCommitTooMany;
  }
  *bad = nblobs;
  CommitLayout& l = *out;
  l = CommitLayout();
  l.nblobs = nblobs;
  l.nshares = (size_t)nshares;
  std::vector<uint32_t> sizes, sub_pre(nblobs + 1, 0);
  for (size_t b = 0; b < nblobs; b++) {
    const uint64_t c = (uint64_t)blobs[b * kCommitReqWords + 2];
    const size_t t = commit_mountain_sizes(c, commit_subtree_width(c, threshold), &sizes);
    sub_pre[b + 1] = sub_pre[b] + (uint32_t)t;
    if (t > l.max_subtrees) l.max_subtrees = (uint32_t)t;
  }
  l.nsub = sizes.size();
  for (uint32_t s : sizes) l.nwork += s >= 2;
  l.o_blob = 0;
  l.o_share_pre = l.o_blob + kCommitBlobWords * nblobs;
  l.o_sub_pre = l.o_share_pre + nblobs + 1;
  l.o_sub = l.o_sub_pre + nblobs + 1;
  l.o_work = l.o_sub + kCommitSubWords * l.nsub;
  l.words.assign(l.o_work + l.nwork, 0);
  uint32_t* w = l.words.data();
  uint32_t leaf = 0;
  size_t s = 0, wk = 0;
  for (size_t b = 0; b < nblobs; b++) {
    const int64_t* r = blobs + b * kCommitReqWords;
    w[l.o_blob + kCommitBlobWords * b] = (uint32_t)r[0];
    w[l.o_blob + kCommitBlobWords * b + 1] = (uint32_t)r[1];
    w[l.o_share_pre + b] = leaf;
    w[l.o_sub_pre + b] = sub_pre[b];
    for (; s < sub_pre[b + 1]; s++) {
      uint32_t* q = w + l.o_sub + kCommitSubWords * s;
      q[0] = (uint32_t)b;
      q[1] = leaf;
      q[2] = sizes[s];
      if (sizes[s] >= 2) w[l.o_work + wk++] = (uint32_t)s;
      leaf += sizes[s];
    }
  }
  w[l.o_share_pre + nblobs] = leaf;
  w[l.o_sub_pre + nblobs] = sub_pre[nblobs];
  return kCommitOk;
}

// Workspace carve (bytes, every part 256-B aligned): the table image, the leaf
// records (96 B per share), the odd tree levels (96 B per two shares) and two
// digest arrays of 32 B per subtree for the RFC-6962 levels.
struct CommitCarve {
  size_t o_tables, o_leaves, o_inner, o_dig0, o_dig1, total;
};
inline size_t commit_align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline CommitCarve commit_carve(size_t table_words, size_t nshares, size_t nsub) {
  CommitCarve c;
  c.o_tables = 0;
  c.o_leaves = commit_align256(4 * table_words);
  c.o_inner = c.o_leaves + commit_align256(96 * nshares);
  c.o_dig0 = c.o_inner + commit_align256(96 * (nshares / 2 + 1));
  c.o_dig1 = c.o_dig0 + commit_align256(32 * nsub);
  c.total = c.o_dig1 + commit_align256(32 * nsub);
  return c;
}
// the most table words a call with these totals can need (nsub <= nshares)
inline size_t commit_table_words_max(size_t nblobs, size_t nshares) {
  return (kCommitBlobWords + 2) * nblobs + 2 + (kCommitSubWords + 1) * nshares;
}

}  // namespace dagpu
