// Stand-alone host check of csrc/commit_plan.hpp (tests/test_commit_plan_host.py
// compiles and runs it; no GPU, no HIP).
//   * For every share count 1 .. 16385 and for 65536 and the thresholds 1, 64
//     and 65: the subtree count, the work count and the j-th subtree (size and
//     first leaf) equal commit_mountain_sizes with commit_subtree_width.
//   * The layout executor over a hand-built arena (blocks of 0, 1 and several
//     blobs, a rejected record, a record of another width, records whose
//     blob_off or nblob run past plan_bytes, a plan past the arena, a blob past
//     the square) equals commit_layout's image of the blobs that remain, word
//     for word, with the counts and blob_base; the arena is allocated exactly,
//     so the sanitized build sees any read outside it.
//   * The verdict function: every code, and each precedence pair.
// Prints "OK key=value ...".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "commit_layout.hpp"
#include "commit_plan.hpp"

using namespace dagpu;

static int fail(const char* what, long a = 0, long b = 0, long c = 0) {
  printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
  return 1;
}

struct Blob {
  uint32_t first, count;
};

// a plan that holds a header and a blob table only; returns its offset in the arena
static uint64_t add_plan(std::vector<uint8_t>& arena, uint32_t k, const std::vector<Blob>& blobs, uint32_t* bytes) {
  const uint64_t at = arena.size();
  const uint32_t blob_off = sizeof(SqHdr), total = (uint32_t)sp_up16(blob_off + blobs.size() * kSqBlobWords * 4);
  arena.resize(at + total, 0);
  SqHdr h;
  memset(&h, 0, sizeof h);
  h.magic = kSqMagic;
  h.version = kSqVersion;
  h.k = k;
  h.plan_bytes = total;
  h.nblob = (uint32_t)blobs.size();
  h.blob_off = blob_off;
  memcpy(arena.data() + at, &h, sizeof h);
  for (size_t i = 0; i < blobs.size(); i++) {
    uint32_t rec[kSqBlobWords] = {0};
    rec[8] = blobs[i].first;
    rec[9] = blobs[i].count;
    rec[10] = 1000 + (uint32_t)i;
    rec[11] = blobs[i].count * 400;
    memcpy(arena.data() + at + blob_off + i * kSqBlobWords * 4, rec, sizeof rec);
  }
  *bytes = total;
  return at;
}

static PvOut verdict(uint32_t plan_status, uint32_t block_k, uint32_t st_tx, uint32_t st_word, uint64_t key,
                     int size, uint32_t ext, uint32_t root) {
  PvIn v;
  v.plan_status = plan_status;
  v.block_k = block_k;
  v.k = 16;
  v.st_tx = st_tx;
  v.st_word = st_word;
  v.commit_key = key;
  v.have_size = size >= 0;
  v.size = size >= 0 ? (uint32_t)size : 0;
  v.extend_status = ext;
  v.root_differs = root;
  return pv_block(v);
}
static bool is(const PvOut& o, uint32_t code, uint32_t tx, uint32_t word, uint32_t aux) {
  return o.code == code && o.tx == tx && o.word == word && o.aux == aux;
}

int main() {
  // ---- the mountain range without a vector --------------------------------------
  long checked = 0;
  std::vector<uint32_t> counts;
  for (uint32_t c = 1; c <= 16385; c++) counts.push_back(c);
  counts.push_back(65536);
  for (uint32_t th : {1u, 64u, 65u})
    for (uint32_t c : counts) {
      const uint64_t w = commit_subtree_width(c, th);
      if (cp_subtree_width(c, th) != w) return fail("width", c, th, (long)w);
      std::vector<uint32_t> want;
      commit_mountain_sizes(c, w, &want);
      const uint32_t lw = cp_log2((uint32_t)w);
      if ((1u << lw) != w) return fail("log2", c, th);
      if (cp_subtree_count(c, lw) != want.size()) return fail("subtree count", c, th, (long)want.size());
      uint32_t work = 0, leaf = 0;
      for (uint32_t j = 0; j < want.size(); j++) {
        uint32_t first = ~0u;
        const uint32_t size = cp_subtree(c, lw, j, &first);
        if (size != want[j] || first != leaf) return fail("subtree", c, j, size);
        if (want[j] >= 2) {
          if (work != j) return fail("a one-leaf subtree before a larger one", c, j);
          work++;
        }
        leaf += want[j];
      }
      if (cp_work_count(c, lw) != work) return fail("work count", c, th, work);
      checked++;
    }

  // ---- the layout executor over a hand-built arena --------------------------------
  const uint32_t k = 16, th = 64;
  std::vector<uint8_t> arena;
  std::vector<SpRecord> rec;
  std::vector<std::vector<Blob>> kept;  // the blobs each block contributes
  auto block = [&](uint32_t width, const std::vector<Blob>& blobs, bool counts_in) {
    SpRecord r;
    memset(&r, 0, sizeof r);
    r.plan_off = add_plan(arena, width, blobs, &r.plan_bytes);
    r.k = width;
    r.nblob = (uint32_t)blobs.size();
    rec.push_back(r);
    kept.push_back(counts_in ? blobs : std::vector<Blob>());
  };
  std::vector<Blob> many;
  for (uint32_t i = 0; i < 70; i++) many.push_back({2 * i, 1 + (i % 2)});  // 70 blobs of 1 and 2 shares
  block(16, {}, true);                                                   // 0: no blobs
  block(16, {{3, 65}}, true);                                            // 1: one blob
  block(16, {{0, 1}, {1, 2}, {4, 64}, {70, 129}, {200, 3}}, true);       // 2: several
  block(16, {{0, 5}}, false);                                            // 3: rejected below
  block(8, {{0, 5}, {8, 2}}, false);                                     // 4: another width
  block(16, {{0, 7}, {9, 9}}, false);                                    // 5: blob_off past plan_bytes below
  block(16, {{0, 7}, {9, 9}}, false);                                    // 6: nblob past plan_bytes below
  block(16, many, true);                                                 // 7: 70 blobs
  block(16, {{0, 4}, {250, 7}}, false);                                  // 8: a blob past the square
  block(16, {{0, 200}, {0, 57}}, false);                                 // 9: more than k * k shares together
  block(16, {{0, 4}, {9, 0}}, false);                                    // 10: a blob without a share
  block(16, {{5, 191}}, true);                                           // 11: the last block
  block(16, {{0, 3}}, false);                                            // 12: a plan past the arena below
  const size_t n = rec.size();
  rec[3].status = kSpLayout | 1u << 8;
  rec[3].plan_bytes = 0;
  ((SqHdr*)(arena.data() + rec[5].plan_off))->blob_off = rec[5].plan_bytes + 16;
  ((SqHdr*)(arena.data() + rec[6].plan_off))->nblob = 1u << 20;
  rec[12].plan_bytes += 64;  // the arena ends with this plan
  std::vector<uint8_t> exact(arena);  // capacity == size: a read past the end is a heap overflow
  exact.shrink_to_fit();

  std::vector<int64_t> req;
  std::vector<uint64_t> want_base(1, 0);
  for (size_t i = 0; i < n; i++) {
    for (const Blob& b : kept[i]) {
      req.push_back((int64_t)i);
      req.push_back(b.first);
      req.push_back(b.count);
    }
    want_base.push_back(req.size() / 3);
  }
  CommitLayout lay;
  size_t bad = 0;
  if (commit_layout(k, n, req.size() / 3, req.data(), 0, 256 * 512, 16 * 512, th, &lay, &bad) != kCommitOk)
    return fail("commit_layout refuses the kept blobs", (long)bad);

  std::vector<uint32_t> tables(cp_cap_table_words(k, n), 0xA5A5A5A5u), counts_out(kCpCountWords, 0xA5A5A5A5u);
  std::vector<uint64_t> blob_base(n + 1, ~(uint64_t)0);
  std::vector<CpSums> sums(n), base(n);
  CpArgs a;
  a.arena = exact.data();
  a.arena_cap = exact.size();
  a.rec = rec.data();
  a.n = (uint32_t)n;
  a.k = k;
  a.threshold = th;
  a.sums = sums.data();
  a.base = base.data();
  a.tables = tables.data();
  a.counts = counts_out.data();
  a.blob_base = blob_base.data();
  cp_layout_host(a);
  const uint32_t want_counts[kCpCountWords] = {(uint32_t)lay.nblobs, (uint32_t)lay.nshares, (uint32_t)lay.nsub,
                                               (uint32_t)lay.nwork, lay.max_subtrees, 0, 0, 0};
  for (uint32_t j = 0; j < kCpCountWords; j++)
    if (counts_out[j] != want_counts[j]) return fail("counts", j, counts_out[j], want_counts[j]);
  if (blob_base != want_base) return fail("blob_base");
  const CpOffsets o = cp_offsets(counts_out[0], counts_out[2], counts_out[3]);
  if (o.words != lay.words.size() || o.share_pre != lay.o_share_pre || o.sub_pre != lay.o_sub_pre ||
      o.sub != lay.o_sub || o.work != lay.o_work)
    return fail("offsets", (long)o.words, (long)lay.words.size());
  if (o.words > tables.size()) return fail("image past the capacity");
  for (size_t i = 0; i < lay.words.size(); i++)
    if (tables[i] != lay.words[i]) return fail("image word", (long)i, tables[i], lay.words[i]);
  for (size_t i = lay.words.size(); i < tables.size(); i++)
    if (tables[i] != 0xA5A5A5A5u) return fail("a store past the image", (long)i);
  if (lay.nshares > cp_cap_items(k, n) || lay.nsub > cp_cap_items(k, n) || 2 * lay.nwork > cp_cap_items(k, n))
    return fail("capacities");

  // ---- the verdict ---------------------------------------------------------------
  const uint32_t none = kPvNone, signer = 14, pfb = 24 | 1u << 8;
  const uint64_t no = kPvNoKey;
  int verdicts = 0;
  auto expect = [&](const char* what, const PvOut& got, uint32_t code, uint32_t tx, uint32_t word, uint32_t aux) {
    if (!is(got, code, tx, word, aux)) {
      printf("FAIL verdict %s: {%u, %u, %u, %u}\n", what, got.code, got.tx, got.word, got.aux);
      return false;
    }
    verdicts++;
    return true;
  };
  const uint64_t mis9 = pv_commit_key(9, 1, kPvCommitMismatch), push9 = pv_commit_key(9, 1, kPvCommitPushOrder | 1);
  // every code
  if (!expect("accept", verdict(0, 16, none, 0, no, 16, 0, 0), kPvAccept, none, 0, 0)) return 1;
  if (!expect("accept, nothing given", verdict(0, 16, none, 0, no, -1, 0, 0), kPvAccept, none, 0, 0)) return 1;
  if (!expect("pfb", verdict(0, 16, 3, pfb, no, 16, 0, 0), kPvNonBlobTxHasPfb, 3, pfb, 0)) return 1;
  if (!expect("stateless", verdict(0, 16, 7, signer, no, 16, 0, 0), kPvInvalidBlobTx, 7, signer, 0)) return 1;
  if (!expect("push order", verdict(0, 16, none, 0, push9, 16, 0, 0), kPvCalculateCommitment, 9, 0, 1)) return 1;
  if (!expect("mismatch", verdict(0, 16, none, 0, mis9, 16, 0, 0), kPvInvalidShareCommitment, 9, 0, 1)) return 1;
  if (!expect("construct", verdict(0x104, 0, none, 0, no, -1, 0, 0), kPvConstructFailed, none, 0x104, 0)) return 1;
  if (!expect("size", verdict(0, 16, none, 0, no, 32, 0, 0), kPvSquareSizeDiffers, none, 0, 16)) return 1;
  if (!expect("not judged", verdict(0, 8, none, 0, no, -1, 0, 0), kPvNotJudged, none, 0, 0)) return 1;
  if (!expect("extend", verdict(0, 16, none, 0, no, 16, 5, 1), kPvExtendFailed, none, 0, 0)) return 1;
  if (!expect("root", verdict(0, 16, none, 0, no, 16, 0, 1), kPvDataRootDiffers, none, 0, 0)) return 1;
  // precedence: the lowest tx over both rule sets
  if (!expect("stateless 12, mismatch 9", verdict(0, 16, 12, signer, mis9, 16, 0, 1), kPvInvalidShareCommitment, 9, 0, 1))
    return 1;
  if (!expect("stateless 7, mismatch 9", verdict(0, 16, 7, signer, mis9, 16, 0, 1), kPvInvalidBlobTx, 7, signer, 0))
    return 1;
  if (!expect("one tx both ways", verdict(0, 16, 9, signer, mis9, 16, 0, 1), kPvInvalidBlobTx, 9, signer, 0)) return 1;
  if (!expect("pfb 12, mismatch 9", verdict(0, 16, 12, pfb, mis9, 16, 0, 0), kPvInvalidShareCommitment, 9, 0, 1)) return 1;
  // within a tx: the lower blob, and its push order before its mismatch
  if (pv_commit_key(9, 0, kPvCommitMismatch) >= pv_commit_key(9, 1, kPvCommitPushOrder)) return fail("blob order");
  if (push9 >= mis9 || mis9 >= pv_commit_key(10, 0, kPvCommitPushOrder)) return fail("key order");
  if (pv_commit_key(none, none, kPvCommitMismatch) == no) return fail("an untied row's key is the empty key");
  if (!expect("untied row", verdict(0, 16, none, 0, pv_commit_key(none, none, 1), 16, 0, 0), kPvInvalidShareCommitment,
              none, 0, 0x7FFFFFFE))
    return 1;
  // the tx loop before Construct, Construct before the size, the size before NOT_JUDGED, then extend, then the root
  if (!expect("rejected, stateless", verdict(0x104, 0, 4, signer, no, 16, 0, 0), kPvInvalidBlobTx, 4, signer, 0)) return 1;
  if (!expect("mismatch, wrong size", verdict(0, 16, none, 0, mis9, 32, 1, 1), kPvInvalidShareCommitment, 9, 0, 1))
    return 1;
  if (!expect("rejected, wrong size", verdict(0x104, 0, none, 0, no, 16, 0, 0), kPvConstructFailed, none, 0x104, 0))
    return 1;
  if (!expect("other width, stateless", verdict(0, 8, 2, signer, no, 8, 0, 0), kPvInvalidBlobTx, 2, signer, 0)) return 1;
  if (!expect("other width, wrong size", verdict(0, 8, none, 0, no, 16, 0, 0), kPvSquareSizeDiffers, none, 0, 8)) return 1;
  if (!expect("other width, right size", verdict(0, 8, none, 0, no, 8, 0, 0), kPvNotJudged, none, 0, 0)) return 1;
  if (!expect("other width, bad root", verdict(0, 8, none, 0, no, -1, 1, 1), kPvNotJudged, none, 0, 0)) return 1;
  if (!expect("size before extend", verdict(0, 16, none, 0, no, 4, 1, 1), kPvSquareSizeDiffers, none, 0, 16)) return 1;

  // the two passes over rows: blocks 0..2 own rows [0,2), [2,2), [2,5)
  {
    SpRecord r3[3];
    memset(r3, 0, sizeof r3);
    for (auto& r : r3) r.k = 16, r.plan_bytes = 96;
    const uint32_t block_status[6] = {none, 0, none, 0, 12, signer};
    const int32_t blob_status[5] = {0, 0, 1, 0, 1};
    const uint32_t row_tx[10] = {0, 0, 1, 0, 11, 1, 9, 0, 9, 1};
    const uint64_t bb[4] = {0, 2, 2, 5};
    unsigned long long key[3] = {kPvNoKey, kPvNoKey, kPvNoKey};
    uint32_t out[12];
    PvArgs p;
    p.rec = r3;
    p.block_status = block_status;
    p.blob_status = blob_status;
    p.row_tx = row_tx;
    p.blob_base = bb;
    p.extend_status = nullptr;
    p.dah = nullptr;
    p.hashes = nullptr;
    p.sizes = nullptr;
    p.key = key;
    p.verdicts = out;
    p.n = 3;
    p.k = 16;
    pv_host(p);
    const uint32_t want[12] = {kPvAccept, none, 0, 0, kPvAccept, none, 0, 0, kPvInvalidShareCommitment, 9, 0, 1};
    if (memcmp(out, want, sizeof want)) return fail("pv_host", out[8], out[9], out[11]);
    if (pv_row_block(bb, 3, 1) != 0 || pv_row_block(bb, 3, 2) != 2 || pv_row_block(bb, 3, 4) != 2) return fail("row block");
  }
  printf("OK checked=%ld blocks=%zu blobs=%zu shares=%zu subtrees=%zu work=%zu maxtrees=%u verdicts=%d\n", checked, n,
         lay.nblobs, lay.nshares, lay.nsub, lay.nwork, lay.max_subtrees, verdicts);
  return 0;
}
