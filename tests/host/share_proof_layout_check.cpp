// Stand-alone host check of csrc/share_proof_layout.hpp
// (tests/test_share_proof_layout_host.py compiles and runs it; no GPU, no HIP).
//   * For k = 1, 2, 4, 8 and every range [start, end) of the ODS: the row split
//     of share_proof_requests equals a loop written straight from
//     pkg/proof/proof.go:63-67, 127-140, and the spans are its prefix sums.
//   * A mixed batch of 5-word requests over several squares: node_off and
//     leaf_off are the prefix sums, the nmt and merkle descriptors have the
//     verifiers' formats, the packed words unpack to the request.
//   * One refusal per invalid class, for the 3-word and the 5-word requests,
//     with nothing written.
//   * DAH-tree addressing: levels are packed one after another and the aunt of
//     leaf j at level L is node (L, (j >> L) ^ 1), checked against a tree built
//     level by level; the store's regions do not overlap and are 256-B aligned.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../celestia-app_amd/csrc/share_proof_layout.hpp"

using namespace dagpu;

static int fail(const char* what, long a = 0, long b = 0, long c = 0) {
  printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
  return 1;
}

struct RowReq {
  int64_t row, start, end;
};

// proof.go:63-67: startRow = start / k, endRow = (end - 1) / k, startLeaf =
// start % k, endLeaf = (end - 1) % k; proof.go:127-140: for each row the range
// runs from startLeaf (first row) or 0 to endLeaf (last row) or k - 1, and
// ProveRange takes [startLeafPos, endLeafPos + 1).
static std::vector<RowReq> reference_split(int64_t k, int64_t start, int64_t end) {
  const int64_t start_row = start / k, end_row = (end - 1) / k;
  const int64_t start_leaf = start % k, end_leaf = (end - 1) % k;
  std::vector<RowReq> out;
  for (int64_t i = start_row; i <= end_row; i++) {
    int64_t start_leaf_pos = 0, end_leaf_pos = k - 1;
    if (i == start_row) start_leaf_pos = start_leaf;
    if (i == end_row) end_leaf_pos = end_leaf;
    out.push_back({i, start_leaf_pos, end_leaf_pos + 1});
  }
  return out;
}

int main() {
  long ranges = 0, rows = 0;
  for (uint32_t k = 1; k <= 8; k *= 2) {
    const int64_t kk = (int64_t)k * k;
    // all ranges of the square in one call, on square (start % 3) of 3
    std::vector<int64_t> sreq;
    std::vector<RowReq> want;
    std::vector<int64_t> want_span{0};
    for (int64_t s = 0; s < kk; s++)
      for (int64_t e = s + 1; e <= kk; e++) {
        sreq.insert(sreq.end(), {s % 3, s, e});
        const std::vector<RowReq> r = reference_split(k, s, e);
        want.insert(want.end(), r.begin(), r.end());
        want_span.push_back((int64_t)want.size());
      }
    const size_t n = sreq.size() / 3;
    std::vector<int64_t> req(want.size() * kProveSqReqWords, -7), span(n + 1, -7);
    size_t n_req = 0;
    if (!share_proof_requests(k, 3, n, sreq.data(), req.data(), want.size(), span.data(), &n_req))
      return fail("split refused", k);
    if (n_req != want.size()) return fail("split count", k, (long)n_req, (long)want.size());
    for (size_t i = 0; i <= n; i++)
      if (span[i] != want_span[i]) return fail("span", k, (long)i);
    for (size_t i = 0; i < n; i++)
      for (int64_t j = span[i]; j < span[i + 1]; j++) {
        const int64_t* r = &req[j * kProveSqReqWords];
        if (r[0] != sreq[3 * i] || r[1] != 0 || r[2] != want[j].row || r[3] != want[j].start ||
            r[4] != want[j].end)
          return fail("split row", k, (long)i, (long)j);
        if (r[3] < 0 || r[3] >= r[4] || r[4] > (int64_t)k) return fail("split outside Q0", k, (long)i, (long)j);
      }
    // one row too few: refused, nothing written
    if (n_req) {
      std::vector<int64_t> r2(req.size(), -7), s2(n + 1, -7);
      size_t nr2 = 99;
      if (share_proof_requests(k, 3, n, sreq.data(), r2.data(), n_req - 1, s2.data(), &nr2))
        return fail("cap not refused", k);
      for (int64_t v : r2)
        if (v != -7) return fail("cap wrote requests", k);
      for (int64_t v : s2)
        if (v != -7) return fail("cap wrote spans", k);
      if (nr2 != 99) return fail("cap wrote n_req", k);
    }
    ranges += (long)n;
    rows += (long)n_req;
  }

  long refused = 0;
  {  // 3-word refusals, k = 4, 2 squares: one bad range among valid ones
    const int64_t bad[][3] = {{2, 0, 1}, {-1, 0, 1}, {0, -1, 3}, {0, 3, 3}, {0, 5, 4}, {1, 0, 17}};
    for (const auto& b : bad) {
      const int64_t sreq[9] = {0, 0, 16, b[0], b[1], b[2], 1, 3, 9};
      int64_t req[64 * kProveSqReqWords], span[4] = {-7, -7, -7, -7};
      for (int64_t& v : req) v = -7;
      size_t n_req = 99;
      if (share_proof_requests(4, 2, 3, sreq, req, 64, span, &n_req)) return fail("3-word not refused", b[0], b[1], b[2]);
      for (int64_t v : req)
        if (v != -7) return fail("3-word refusal wrote", b[0], b[1], b[2]);
      if (span[0] != -7 || span[3] != -7 || n_req != 99) return fail("3-word refusal wrote spans", b[0], b[1], b[2]);
      refused++;
    }
  }

  long batch = 0;
  {  // mixed batch over 3 squares of k = 4 (w = 8, m = 3, 16 DAH leaves, 4 aunts)
    const uint32_t k = 4;
    const int64_t w = 8;
    std::vector<int64_t> req;
    for (int64_t i = 0; i < 3 * 2 * w; i++) {
      const int64_t sq = (i * 7) % 3, axis = (i / 3) % 2, index = (i * 5) % w;
      const int64_t s = i % w, e = s + 1 + (i * 3) % (w - s);
      req.insert(req.end(), {sq, axis, index, s, e});
    }
    const size_t n = req.size() / kProveSqReqWords;
    ProveLayout lay;
    size_t bad = 99;
    if (prove_squares_layout(k, 3, n, req.data(), ~(size_t)0, true, ~(size_t)0, &lay, &bad) != kProveOk)
      return fail("batch refused", (long)bad);
    int64_t nodes = 0, leaves = 0;
    for (size_t i = 0; i < n; i++) {
      const int64_t* r = &req[i * kProveSqReqWords];
      if (lay.node_off[i] != nodes || lay.leaf_off[i] != leaves) return fail("prefix sums", (long)i);
      nodes += prove_node_count(3, (uint32_t)r[3], (uint32_t)r[4]);
      leaves += r[4] - r[3];
    }
    if (lay.node_off[n] != nodes || lay.leaf_off[n] != leaves || lay.n_nodes != nodes || lay.n_leaves != leaves)
      return fail("totals");
    std::vector<int64_t> desc(n * kProveDescWords), mdesc(n * kMerkleDescWords);
    prove_squares_fill_desc(n, req.data(), lay, desc.data());
    prove_squares_fill_mdesc(k, n, req.data(), mdesc.data());
    for (size_t i = 0; i < n; i++) {
      const int64_t* r = &req[i * kProveSqReqWords];
      const int64_t* d = &desc[i * kProveDescWords];
      const int64_t* md = &mdesc[i * kMerkleDescWords];
      if (d[0] != r[3] || d[1] != r[4] || d[2] != r[4] - r[3] || d[3] != lay.leaf_off[i] ||
          d[4] != lay.node_off[i + 1] - lay.node_off[i] || d[5] != lay.node_off[i] || d[6] != (int64_t)i ||
          d[7] != (int64_t)i)
        return fail("nmt descriptor", (long)i);
      if (md[0] != r[1] * w + r[2] || md[1] != 2 * w || md[2] != 4 || md[3] != 4 * (int64_t)i ||
          md[4] != (int64_t)i || md[5] != r[0])
        return fail("merkle descriptor", (long)i);
      int64_t packed[2];
      prove_squares_pack_req(r, packed);
      const uint64_t v = (uint64_t)packed[0];
      if ((int64_t)(v & 0xFFFF) != r[1] || (int64_t)((v >> 16) & 0xFFFF) != r[2] ||
          (int64_t)((v >> 32) & 0xFFFF) != r[3] || (int64_t)((v >> 48) & 0xFFFF) != r[4] || packed[1] != r[0])
        return fail("packed request", (long)i);
      batch++;
    }
    // one refusal per invalid class, the offending request named; capacities
    struct Bad {
      int64_t r[5];
      int want;
    };
    const Bad bads[] = {{{3, 0, 0, 0, 1}, kProveBadSquare}, {{-1, 0, 0, 0, 1}, kProveBadSquare},
                        {{0, 2, 0, 0, 1}, kProveBadAxis},   {{0, -1, 0, 0, 1}, kProveBadAxis},
                        {{0, 0, 8, 0, 1}, kProveBadIndex},  {{0, 1, -1, 0, 1}, kProveBadIndex},
                        {{0, 0, 0, -1, 1}, kProveBadRange}, {{0, 0, 0, 2, 2}, kProveBadRange},
                        {{0, 0, 0, 3, 9}, kProveBadRange}};
    for (const Bad& b : bads) {
      std::vector<int64_t> r2 = req;
      const size_t at = 5;
      memcpy(&r2[at * kProveSqReqWords], b.r, sizeof b.r);
      ProveLayout l2;
      size_t where = 99;
      if (prove_squares_layout(k, 3, n, r2.data(), ~(size_t)0, true, ~(size_t)0, &l2, &where) != b.want || where != at)
        return fail("5-word refusal", b.want, (long)where);
      refused++;
    }
    ProveLayout l3;
    size_t where = 99;
    if (prove_squares_layout(k, 3, n, req.data(), (size_t)nodes - 1, true, ~(size_t)0, &l3, &where) != kProveNodesCap ||
        where != n)
      return fail("nodes_cap");
    if (prove_squares_layout(k, 3, n, req.data(), (size_t)nodes, true, (size_t)leaves - 1, &l3, &where) !=
            kProveSharesCap || where != n)
      return fail("shares_cap");
    if (prove_squares_layout(k, 3, n, req.data(), (size_t)nodes, false, 0, &l3, &where) != kProveOk)
      return fail("shares_cap checked without shares");
    refused += 2;
  }

  long aunts = 0;
  for (uint32_t k = 1; k <= 8; k *= 2) {
    // a tree of node ids built level by level: node (L, p) = id of its leaf span
    const long leaves = 4L * k;
    int m = 0;
    while ((1L << m) < leaves) m++;
    long off = 0;
    for (int L = 0; L <= m; L++) {
      if (dah_level_off(leaves, L) != off) return fail("level offset", k, L);
      off += leaves >> L;
    }
    if (off != 2 * leaves - 1) return fail("tree size", k);
    for (long j = 0; j < leaves; j++)
      for (int L = 0; L < m; L++) {
        // the aunt at level L is the sibling of j's ancestor at that level
        const long anc = j >> L, sib = anc ^ 1;
        if (dah_aunt_at(leaves, j, L) != dah_level_off(leaves, L) + sib) return fail("aunt", k, j, L);
        if (sib >> 1 != anc >> 1 || sib == anc || sib >= (leaves >> L)) return fail("aunt not a sibling", k, j, L);
        aunts++;
      }
    for (size_t n = 1; n <= 3; n++) {
      ProofStoreLayout l;
      if (!proof_store_layout(k, n, &l)) return fail("store layout", k, (long)n);
      const size_t w = 2 * (size_t)k;
      size_t recs = 0;
      for (size_t per = w; per >= 1; per >>= 1) recs += w * per;
      if (l.row_bytes != recs * 96 || l.col_bytes != (recs - w * w) * 96 || l.dah_bytes != (8 * (size_t)k - 1) * 32)
        return fail("store sizes", k, (long)n);
      if (l.col_off % 256 || l.dah_off % 256 || l.col_off < n * l.row_bytes ||
          l.dah_off < l.col_off + n * l.col_bytes || l.total < l.dah_off + n * l.dah_bytes)
        return fail("store regions", k, (long)n);
    }
  }
  printf("OK ranges=%ld rows=%ld batch=%ld refused=%ld aunts=%ld\n", ranges, rows, batch, refused, aunts);
  return 0;
}
