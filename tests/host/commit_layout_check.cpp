// Stand-alone host check of csrc/commit_layout.hpp (tests/test_commit_layout_host.py
// compiles and runs it; no GPU, no HIP).
//   * For every share count 1 .. 16385 and for 65536 (threshold 64):
//     commit_subtree_width and commit_mountain_sizes equal an independent
//     restatement (the width through a floating square root as the Go code
//     takes it, the sizes as whole trees plus the set bits of the rest).
//   * A batch of mixed blobs over three squares: the prefix sums and the
//     subtree records cover every share once and in order, the work list names
//     exactly the subtrees of two leaves or more, and the carve keeps every
//     part of the workspace apart and inside the advertised size.
//   * Each refusal class is refused with its own reason and names the blob.
// Prints "OK key=value ..." for the Python side to assert spot values.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../../celestia-app_amd/csrc/commit_layout.hpp"

using namespace dagpu;

static int fail(const char* what, long a = 0, long b = 0, long c = 0) {
  printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
  return 1;
}

static uint64_t pow2_at_least(uint64_t v) {
  uint64_t r = 1;
  while (r < v) r *= 2;
  return r;
}

// SubTreeWidth as blob_share_commitment_rules.go states it
static uint64_t ref_width(uint64_t count, uint64_t threshold) {
  uint64_t s = count / threshold;
  if (count % threshold != 0) s++;
  s = pow2_at_least(s);
  const uint64_t min_sq = pow2_at_least((uint64_t)ceil(sqrt((double)count)));
  return s < min_sq ? s : min_sq;
}

// the mountain range: count / w whole trees, then the binary digits of the rest
static std::vector<uint32_t> ref_sizes(uint64_t count, uint64_t w) {
  std::vector<uint32_t> out(count / w, (uint32_t)w);
  const uint64_t rest = count % w;
  for (int b = 62; b >= 0; b--)
    if ((rest >> b) & 1) out.push_back((uint32_t)1 << b);
  return out;
}

static std::string join_tail(const std::vector<uint32_t>& v, size_t n) {
  std::string s;
  for (size_t i = v.size() > n ? v.size() - n : 0; i < v.size(); i++) s += (s.empty() ? "" : ",") + std::to_string(v[i]);
  return s;
}

int main() {
  std::string fields;
  size_t max_trees = 0;
  long checked = 0;
  std::vector<uint64_t> counts;
  for (uint64_t c = 1; c <= 16385; c++) counts.push_back(c);
  counts.push_back(65536);
  for (uint64_t c : counts) {
    const uint64_t w = commit_subtree_width(c, 64);
    if (w != ref_width(c, 64)) return fail("width", (long)c, (long)w, (long)ref_width(c, 64));
    std::vector<uint32_t> got;
    const size_t t = commit_mountain_sizes(c, w, &got);
    const std::vector<uint32_t> want = ref_sizes(c, w);
    if (t != got.size() || got != want) return fail("mountain sizes", (long)c, (long)t, (long)want.size());
    uint64_t sum = 0;
    for (uint32_t s : got) {
      if (s == 0 || (s & (s - 1)) || s > w) return fail("size not a power of two <= w", (long)c, (long)s);
      sum += s;
    }
    if (sum != c) return fail("sizes do not add up", (long)c, (long)sum);
    if (c <= 16384 && t > max_trees) max_trees = t;
    checked++;
    for (uint64_t spot : {65, 129, 191, 2049, 4097, 16383, 16385, 65536})
      if (c == spot)
        fields += " w" + std::to_string(c) + "=" + std::to_string(w) + " t" + std::to_string(c) + "=" +
                  std::to_string(t) + " tail" + std::to_string(c) + "=" + join_tail(got, 8);
  }
  // other thresholds agree with the restatement too
  for (uint64_t th : {1, 2, 7, 64, 100})
    for (uint64_t c = 1; c <= 600; c++)
      if (commit_subtree_width(c, th) != ref_width(c, th)) return fail("width at threshold", (long)c, (long)th);

  // ---- a batch of mixed blobs ---------------------------------------------
  const uint32_t k = 16;
  const size_t n = 3;
  const int64_t req[][3] = {{0, 0, 1},  {2, 5, 64},  {1, 3, 65},  {0, 17, 127}, {2, 100, 129}, {1, 60, 191},
                            {0, 0, 256}, {1, 255, 1}, {2, 13, 3}, {0, 31, 2},   {0, 0, 1}};
  const size_t nb = sizeof req / sizeof req[0];
  CommitLayout lay;
  size_t bad = 99;
  if (commit_layout(k, n, nb, &req[0][0], 0x1000, 256 * 512, 16 * 512, 64, &lay, &bad) != kCommitOk || bad != nb)
    return fail("batch refused", (long)bad);
  const uint32_t* w = lay.words.data();
  if (lay.nblobs != nb || lay.words.size() != lay.o_work + lay.nwork) return fail("layout totals");
  uint32_t leaf = 0, sub = 0, work = 0, most = 0;
  for (size_t b = 0; b < nb; b++) {
    if (w[lay.o_blob + 2 * b] != (uint32_t)req[b][0] || w[lay.o_blob + 2 * b + 1] != (uint32_t)req[b][1])
      return fail("blob record", (long)b);
    if (w[lay.o_share_pre + b] != leaf || w[lay.o_sub_pre + b] != sub) return fail("prefix sums", (long)b);
    const std::vector<uint32_t> want = ref_sizes((uint64_t)req[b][2], ref_width((uint64_t)req[b][2], 64));
    for (uint32_t s : want) {
      const uint32_t* q = w + lay.o_sub + 3 * sub;
      if (q[0] != b || q[1] != leaf || q[2] != s) return fail("subtree record", (long)b, (long)sub, (long)q[1]);
      if (s >= 2) {
        if (work >= lay.nwork || w[lay.o_work + work] != sub) return fail("work list", (long)sub);
        work++;
      }
      leaf += s;
      sub++;
    }
    if (want.size() > most) most = (uint32_t)want.size();
    if (leaf != w[lay.o_share_pre + b] + (uint32_t)req[b][2]) return fail("blob not covered", (long)b);
  }
  if (w[lay.o_share_pre + nb] != leaf || w[lay.o_sub_pre + nb] != sub || lay.nshares != leaf || lay.nsub != sub ||
      lay.nwork != work || lay.max_subtrees != most)
    return fail("totals", (long)leaf, (long)sub, (long)work);
  const CommitCarve cv = commit_carve(lay.words.size(), lay.nshares, lay.nsub);
  if (cv.o_tables + 4 * lay.words.size() > cv.o_leaves || cv.o_leaves + 96 * lay.nshares > cv.o_inner ||
      cv.o_inner + 96 * (lay.nshares / 2 + 1) > cv.o_dig0 || cv.o_dig0 + 32 * lay.nsub > cv.o_dig1 ||
      cv.o_dig1 + 32 * lay.nsub > cv.total)
    return fail("carve overlaps");
  if ((cv.o_leaves | cv.o_inner | cv.o_dig0 | cv.o_dig1) & 15) return fail("carve misaligned");
  const size_t cap = commit_carve(commit_table_words_max(nb, lay.nshares), lay.nshares, lay.nshares).total;
  if (lay.words.size() > commit_table_words_max(nb, lay.nshares) || cv.total > cap) return fail("advertised size");
  // every subtree's window of the odd levels lies apart from its neighbours'
  uint32_t inner_end = 0;
  for (uint32_t s = 0; s < sub; s++) {
    const uint32_t* q = w + lay.o_sub + 3 * s;
    if (q[2] < 2) continue;
    if ((q[1] >> 1) < inner_end) return fail("inner windows overlap", (long)s);
    inner_end = (q[1] >> 1) + q[2] / 2;
  }
  if (inner_end > lay.nshares / 2 + 1) return fail("inner window past the array", (long)inner_end);

  // ---- refusals --------------------------------------------------------------
  int refused = 0;
  auto refuse = [&](const char* what, CommitCheck want, size_t want_bad, uint32_t kk, size_t nn, size_t nblobs,
                    const int64_t* r, uint64_t base, size_t stride, size_t pitch, uint32_t th) {
    CommitLayout l;
    size_t at = 99;
    const CommitCheck got = commit_layout(kk, nn, nblobs, r, base, stride, pitch, th, &l, &at);
    if (got != want || at != want_bad || !commit_check_text(got)[0]) {
      printf("FAIL refusal %s: got %d at %zu\n", what, (int)got, at);
      return false;
    }
    refused++;
    return true;
  };
  const int64_t ok2[][3] = {{0, 0, 4}, {1, 250, 6}};
  const int64_t* g = &ok2[0][0];
  if (commit_layout(16, 2, 2, g, 0, 131072, 8192, 64, &lay, &bad) != kCommitOk) return fail("good pair refused");
  if (!refuse("k not a power of two", kCommitBadWidth, 2, 12, 2, 2, g, 0, 131072, 8192, 64)) return 1;
  if (!refuse("k zero", kCommitBadWidth, 2, 0, 2, 2, g, 0, 131072, 8192, 64)) return 1;
  if (!refuse("k 2048", kCommitWideSquare, 2, 2048, 2, 2, g, 0, (size_t)1 << 31, 2048 * 512, 64)) return 1;
  if (!refuse("threshold 0", kCommitBadThreshold, 2, 16, 2, 2, g, 0, 131072, 8192, 0)) return 1;
  if (!refuse("short pitch", kCommitBadPitch, 2, 16, 2, 2, g, 0, 131072, 8192 - 16, 64)) return 1;
  if (!refuse("base misaligned", kCommitMisaligned, 2, 16, 2, 2, g, 8, 131072, 8192, 64)) return 1;
  if (!refuse("stride misaligned", kCommitMisaligned, 2, 16, 2, 2, g, 0, 131072 + 4, 8192, 64)) return 1;
  if (!refuse("pitch misaligned", kCommitMisaligned, 2, 16, 2, 2, g, 0, 131072, 8192 + 8, 64)) return 1;
  const int64_t sq_hi[][3] = {{0, 0, 4}, {2, 250, 6}}, sq_neg[][3] = {{-1, 0, 4}, {1, 250, 6}};
  if (!refuse("square past n", kCommitBadSquare, 1, 16, 2, 2, &sq_hi[0][0], 0, 131072, 8192, 64)) return 1;
  if (!refuse("square negative", kCommitBadSquare, 0, 16, 2, 2, &sq_neg[0][0], 0, 131072, 8192, 64)) return 1;
  const int64_t c0[][3] = {{0, 0, 4}, {1, 250, 0}}, cneg[][3] = {{0, 0, -3}, {1, 250, 6}};
  if (!refuse("count zero", kCommitBadCount, 1, 16, 2, 2, &c0[0][0], 0, 131072, 8192, 64)) return 1;
  if (!refuse("count negative", kCommitBadCount, 0, 16, 2, 2, &cneg[0][0], 0, 131072, 8192, 64)) return 1;
  const int64_t past[][3] = {{0, 0, 4}, {1, 250, 7}}, fneg[][3] = {{0, -1, 4}, {1, 250, 6}},
                huge[][3] = {{0, 0, 4}, {1, INT64_MAX - 2, 6}}, whole[][3] = {{0, 0, 257}, {1, 250, 6}};
  if (!refuse("range past the square", kCommitBadRange, 1, 16, 2, 2, &past[0][0], 0, 131072, 8192, 64)) return 1;
  if (!refuse("first negative", kCommitBadRange, 0, 16, 2, 2, &fneg[0][0], 0, 131072, 8192, 64)) return 1;
  if (!refuse("first overflows", kCommitBadRange, 1, 16, 2, 2, &huge[0][0], 0, 131072, 8192, 64)) return 1;
  if (!refuse("count above k*k", kCommitBadRange, 0, 16, 2, 2, &whole[0][0], 0, 131072, 8192, 64)) return 1;
  // no blobs: the geometry is still checked, and a good one passes
  if (!refuse("no blobs, bad pitch", kCommitBadPitch, 0, 16, 2, 0, nullptr, 0, 131072, 16, 64)) return 1;
  if (commit_layout(16, 2, 0, nullptr, 0, 131072, 8192, 64, &lay, &bad) != kCommitOk || lay.nshares || lay.nsub)
    return fail("empty batch");
  // 2^31 shares in one call: 2048 whole squares of k = 1024
  {
    std::vector<int64_t> many(3 * 2048);
    for (size_t i = 0; i < 2048; i++) {
      many[3 * i] = 0;
      many[3 * i + 1] = 0;
      many[3 * i + 2] = 1024 * 1024;
    }
    if (!refuse("2^31 shares", kCommitTooMany, 2047, 1024, 1, 2048, many.data(), 0, 0, 1024 * 512, 64)) return 1;
  }
  printf("OK checked=%ld maxtrees=%zu batch_shares=%u batch_subtrees=%u batch_work=%u refused=%d%s\n", checked,
         max_trees, leaf, sub, work, refused, fields.c_str());
  return 0;
}
