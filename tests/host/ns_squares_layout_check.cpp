// Stand-alone host check of csrc/ns_squares_layout.hpp
// (tests/test_ns_squares_layout_host.py compiles and runs it; no GPU, no HIP).
//   * The packed range word round-trips for w = 2 .. 32768 at the extremes of
//     start and end and for both kinds; outside is the zero word; the four
//     summed quantities are those of the unpacked range.
//   * Hand-made hit tables (absence proofs, whole rows, single cells, several
//     squares and queries): the nmt and merkle descriptors equal a computation
//     written per proof from the definitions, and ns_sq_check_hits accepts
//     exactly the totals of the table.
//   * Each of the four capacities is refused when one short and accepted when
//     exact.
//   * The bound on the node total is the true per-proof maximum (2 log2(2k) - 2,
//     from every range of every tree up to 512 leaves): a batch whose one proof
//     has more than log2(2k) nodes, such as [3, 5) at k = 8, is accepted.
//   * The re-check rejects each malformed hit record and each broken table
//     (order, totals, lane past the batch).
//   * The workspace carve: regions are 256-B aligned, never overlap, lie inside
//     the total, hold what the kernels index, and the total is monotone in
//     n_sq, n_q and proofs_cap; overflowing counts are refused.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../celestia-app_amd/csrc/ns_squares_layout.hpp"

using namespace dagpu;

static int fail(const char* what, long a = 0, long b = 0, long c = 0) {
  printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
  return 1;
}

static int popcount(uint32_t v) {
  int c = 0;
  for (; v; v >>= 1) c += v & 1;
  return c;
}

struct Hit {
  int32_t q, sq, row, kind, start, end;
};

static std::vector<uint32_t> records(const std::vector<Hit>& hits, size_t n_sq, uint32_t w) {
  std::vector<uint32_t> rec;
  for (const Hit& h : hits) {
    rec.push_back((uint32_t)(((uint64_t)h.q * n_sq + h.sq) * w + h.row));
    rec.push_back(ns_sq_pack(h.kind, (uint32_t)h.start, (uint32_t)h.end));
  }
  return rec;
}

int main() {
  long words = 0, tables = 0, proofs = 0, rejected = 0, carves = 0;

  // ---- pack / unpack ----
  if (ns_sq_pack(0, 0, 0) != 0) return fail("outside word");
  for (uint32_t w = 2; w <= 32768; w *= 2) {
    const int m = prove_log2(w);
    const uint32_t starts[] = {0, 1, w / 2 - 1 + (w == 2), w / 2, w - 2, w - 1};
    for (uint32_t s : starts) {
      if (s >= w) continue;
      const uint32_t ends[] = {s + 1, s + 2, w / 2, w - 1, w};
      for (uint32_t e : ends) {
        if (e <= s || e > w) continue;
        for (int kind = 1; kind <= 2; kind++) {
          const uint32_t v = ns_sq_pack(kind, s, e);
          int k2;
          uint32_t s2, e2;
          ns_sq_unpack(v, &k2, &s2, &e2);
          if (v == 0 || k2 != kind || s2 != s || e2 != e) return fail("round trip", w, s, e);
          int64_t q[kNsSqSums];
          ns_sq_quantities(v, m, q);
          if (q[0] != 1 || q[1] != (kind == 2) || q[2] != popcount(s) + m - popcount(e - 1) ||
              q[3] != (kind == 1 ? (int64_t)(e - s) : 0))
            return fail("quantities", w, s, e);
          words++;
        }
      }
    }
  }
  {
    int kind;
    uint32_t s, e;
    ns_sq_unpack(0, &kind, &s, &e);
    int64_t q[kNsSqSums];
    ns_sq_quantities(0, 5, q);
    if (kind != 0 || s != 0 || e != 0 || q[0] || q[1] || q[2] || q[3]) return fail("outside unpack");
    // the largest word: w = 32768, [32767, 32768) and [0, 32768)
    if (ns_sq_pack(2, 32767, 32768) != (2u | (32767u << 2))) return fail("top start");
    if (ns_sq_pack(1, 0, 32768) != (1u | (32767u << 17))) return fail("top length");
  }

  // ---- the most nodes of one proof: every range of every tree up to 512 leaves ----
  for (uint32_t w = 2; w <= 512; w *= 2) {
    const int m = prove_log2(w);
    int most = 0;
    for (uint32_t s = 0; s < w; s++)
      for (uint32_t e = s + 1; e <= w; e++) {
        most = std::max(most, prove_node_count(m, s, e));
        if (e == s + 1 && prove_node_count(m, s, e) != m) return fail("one leaf has m nodes", w, s);
      }
    if (most != ns_sq_max_nodes(m)) return fail("max nodes", w, most, ns_sq_max_nodes(m));
  }

  // ---- descriptors from hand-made tables ----
  struct Table {
    uint32_t k;
    size_t n_q, n_sq;
    std::vector<Hit> hits;
  };
  const std::vector<Table> tabs = {
      // k = 4: an absence proof first, a whole row, single cells, a second square, a second query
      {4, 3, 2, {{0, 0, 0, 2, 3, 4}, {0, 0, 1, 1, 0, 8}, {0, 0, 7, 1, 7, 8}, {0, 1, 0, 1, 0, 1}, {0, 1, 2, 2, 0, 1},
                 {1, 0, 3, 1, 2, 6}, {2, 1, 7, 2, 7, 8}}},
      // k = 1: both rows of three squares
      {1, 2, 3, {{0, 0, 0, 1, 0, 1}, {0, 2, 1, 1, 0, 2}, {1, 1, 0, 2, 1, 2}, {1, 2, 1, 1, 1, 2}}},
      // k = 128: whole parity rows and a run that ends a row
      {128, 2, 64, {{0, 5, 200, 1, 0, 256}, {0, 63, 255, 1, 0, 256}, {1, 0, 0, 1, 100, 128}, {1, 0, 1, 2, 0, 1},
                    {1, 63, 127, 2, 127, 128}}},
      // proofs of more than log2(2k) nodes: two leaves astride a subtree boundary, alone in their batch
      {8, 1, 1, {{0, 0, 0, 1, 3, 5}}},
      {128, 1, 3, {{0, 1, 9, 1, 63, 65}}},
      {128, 1, 1, {{0, 0, 0, 1, 127, 129}}},
      // nothing hits
      {8, 4, 2, {}},
  };
  for (const Table& t : tabs) {
    const uint32_t w = 2 * t.k;
    const int m = prove_log2(w);
    const size_t n = t.hits.size();
    const std::vector<uint32_t> rec = records(t.hits, t.n_sq, w);
    // naive per-proof computation
    std::vector<int64_t> want_d(n * 9), want_m(n * 6);
    int64_t totals[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < n; i++) {
      const Hit& h = t.hits[i];
      int64_t nodes = 0, cells = 0, n_abs = 0;
      for (size_t j = 0; j < i; j++) {
        const Hit& g = t.hits[j];
        nodes += popcount((uint32_t)g.start) + m - popcount((uint32_t)g.end - 1);
        cells += g.kind == 1 ? g.end - g.start : 0;
        n_abs += g.kind == 2;
      }
      const int64_t nn = popcount((uint32_t)h.start) + m - popcount((uint32_t)h.end - 1);
      const int64_t d[9] = {h.start, h.end, h.kind == 1 ? h.end - h.start : 0, cells, nn, nodes, h.q, (int64_t)i,
                            h.kind == 2 ? n_abs : -1};
      memcpy(&want_d[9 * i], d, sizeof d);
      const int64_t md[6] = {h.row, 4 * (int64_t)t.k, m + 1, (int64_t)i * (m + 1), (int64_t)i, h.sq};
      memcpy(&want_m[6 * i], md, sizeof md);
      totals[0]++;
      totals[1] += h.kind == 2;
      totals[2] += nn;
      totals[3] += h.kind == 1 ? h.end - h.start : 0;
    }
    std::vector<int32_t> hits(n * kNsHitWords + 1, 0x5A5A5A5A);
    if (!ns_sq_check_hits(n, rec.data(), t.n_q, t.n_sq, w, totals, hits.data())) return fail("table refused", t.k);
    if (hits[n * kNsHitWords] != 0x5A5A5A5A) return fail("hits overrun", t.k);
    for (size_t i = 0; i < n; i++) {
      const Hit& h = t.hits[i];
      const int32_t want[6] = {h.q, h.sq, h.row, h.kind, h.start, h.end};
      if (memcmp(&hits[6 * i], want, sizeof want)) return fail("hit words", t.k, (long)i);
    }
    std::vector<int64_t> desc(n * 9 + 1, -7), mdesc(n * 6 + 1, -7);
    ns_sq_fill_desc(t.k, n, hits.data(), desc.data(), mdesc.data());
    if (desc[n * 9] != -7 || mdesc[n * 6] != -7) return fail("descriptor overrun", t.k);
    if (n && (memcmp(desc.data(), want_d.data(), n * 9 * 8) || memcmp(mdesc.data(), want_m.data(), n * 6 * 8)))
      return fail("descriptors", t.k);
    ns_sq_fill_desc(t.k, n, hits.data(), desc.data(), nullptr);  // the merkle half is optional
    ns_sq_fill_desc(t.k, n, hits.data(), nullptr, mdesc.data());
    if (!ns_sq_totals_ok(totals, (uint64_t)t.n_q * t.n_sq * w, m, w)) return fail("totals refused", t.k);
    // each total off by one is noticed
    for (int j = 0; j < 4 && n; j++) {
      for (int delta = -1; delta <= 1; delta += 2) {
        int64_t bad[4] = {totals[0], totals[1], totals[2], totals[3]};
        bad[j] += delta;
        if (ns_sq_check_hits(n, rec.data(), t.n_q, t.n_sq, w, bad, hits.data())) return fail("wrong total", t.k, j);
        rejected++;
      }
    }
    // ---- capacities: exact fits, one short does not ----
    if (ns_sq_short_capacity(totals, (size_t)totals[0], (size_t)totals[1], (size_t)totals[2], (size_t)totals[3]) != -1)
      return fail("exact capacity refused", t.k);
    for (int j = 0; j < 4; j++) {
      if (totals[j] == 0) continue;
      size_t cap[4] = {(size_t)totals[0], (size_t)totals[1], (size_t)totals[2], (size_t)totals[3]};
      cap[j]--;
      if (ns_sq_short_capacity(totals, cap[0], cap[1], cap[2], cap[3]) != j) return fail("short capacity", t.k, j);
      rejected++;
    }
    tables++;
    proofs += (long)n;
  }

  // ---- the re-check rejects each malformed record ----
  {
    const size_t n_q = 3, n_sq = 2;
    const uint32_t w = 8;
    const int32_t good[6] = {2, 1, 7, 1, 0, 8};
    if (!ns_sq_hit_ok(good, n_q, n_sq, w)) return fail("good hit refused");
    const std::vector<std::pair<int, int32_t>> bad = {
        {0, -1}, {0, 3},          // query
        {1, -1}, {1, 2},          // square
        {2, -1}, {2, 8},          // row
        {3, 0}, {3, 3}, {3, -1},  // kind
        {4, -1}, {4, 8},          // start < 0, start >= end
        {5, 0}, {5, 9},           // end <= start, end > w
    };
    for (const auto& b : bad) {
      int32_t h[6];
      memcpy(h, good, sizeof h);
      h[b.first] = b.second;
      if (ns_sq_hit_ok(h, n_q, n_sq, w)) return fail("malformed hit accepted", b.first, b.second);
      rejected++;
    }
    const int32_t wide_absent[6] = {0, 0, 0, 2, 1, 3};  // an absence proof is one leaf
    const int32_t empty[6] = {0, 0, 0, 1, 4, 4};
    if (ns_sq_hit_ok(wide_absent, n_q, n_sq, w) || ns_sq_hit_ok(empty, n_q, n_sq, w)) return fail("range accepted");
    rejected += 2;
    // through the device form: kinds 0 and 3, an end past the row, a lane past
    // the batch, lanes out of order and a repeated lane
    const int m = prove_log2(w);
    auto check = [&](const std::vector<uint32_t>& rec) {
      const size_t n = rec.size() / 2;
      int64_t totals[4] = {0, 0, 0, 0};
      for (size_t i = 0; i < n; i++) {
        int64_t q[4];
        ns_sq_quantities(rec[2 * i + 1], m, q);
        for (int j = 0; j < 4; j++) totals[j] += q[j];
      }
      std::vector<int32_t> hits(n * kNsHitWords);
      return ns_sq_check_hits(n, rec.data(), n_q, n_sq, w, totals, hits.data());
    };
    const uint32_t lanes = (uint32_t)(n_q * n_sq * w);
    if (!check({0, ns_sq_pack(1, 0, 8), lanes - 1, ns_sq_pack(2, 7, 8)})) return fail("device form refused");
    const std::vector<std::vector<uint32_t>> bad_rec = {
        {5, 0u},                                           // kind 0
        {5, 3u | (1u << 2)},                               // kind 3
        {5, 1u | (4u << 2) | (4u << 17)},                  // [4, 9) in a row of 8
        {5, 2u | (1u << 2) | (1u << 17)},                  // an absence proof two leaves wide
        {lanes, ns_sq_pack(1, 0, 1)},                      // lane past the batch
        {9, ns_sq_pack(1, 0, 1), 4, ns_sq_pack(1, 0, 1)},  // descending
        {9, ns_sq_pack(1, 0, 1), 9, ns_sq_pack(1, 0, 1)},  // repeated
    };
    for (size_t i = 0; i < bad_rec.size(); i++) {
      if (check(bad_rec[i])) return fail("malformed record accepted", (long)i);
      rejected++;
    }
    // w = 8, m = 3: an absence proof has exactly 3 nodes, a presence proof 0 .. 4 ([3, 5)), so four
    // proofs of which one is absent have 3 .. 15 nodes and at most 24 cells
    if (ns_sq_max_nodes(m) != 4) return fail("max nodes at m = 3");
    const int64_t t_ok[][4] = {{4, 1, 15, 24}, {4, 1, 3, 0}, {1, 0, 4, 2}, {0, 0, 0, 0}};
    for (const auto& t : t_ok)
      if (!ns_sq_totals_ok(t, 48, m, w)) return fail("totals refused", (long)t[0], (long)t[1], (long)t[2]);
    const int64_t t_bad[][4] = {{-1, 0, 0, 0}, {49, 0, 0, 0}, {4, 5, 0, 0}, {4, -1, 0, 0}, {4, 1, 16, 0},
                                {4, 1, 2, 0}, {4, 1, -1, 0}, {4, 1, 12, 25}, {4, 1, 12, -1}, {1, 0, 5, 2}};
    for (const auto& t : t_bad) {
      if (ns_sq_totals_ok(t, 48, m, w)) return fail("totals accepted", (long)t[0], (long)t[1], (long)t[2]);
      rejected++;
    }
  }

  // ---- the workspace carve ----
  {
    const uint32_t ks[] = {1, 2, 8, 128, 8192};
    const size_t nsqs[] = {1, 3, 64}, nqs[] = {0, 1, 257, 1024}, caps[] = {0, 1, 1000, 70000};
    for (uint32_t k : ks) {
      size_t prev_sq = 0;
      for (size_t n_sq : nsqs) {
        size_t prev_q = 0;
        for (size_t n_q : nqs) {
          size_t prev_cap = 0;
          for (size_t cap : caps) {
            NsSqCarve c;
            if (!ns_squares_carve(k, n_sq, n_q, cap, &c)) return fail("carve refused", k, (long)n_sq, (long)n_q);
            const uint64_t w = 2 * (uint64_t)k;
            if (c.lanes != n_q * n_sq * w || c.pairs != n_q * n_sq || c.blocks * 256 < c.lanes ||
                (c.blocks && (c.blocks - 1) * 256 >= c.lanes) || c.chunks * 256 < c.blocks)
              return fail("carve counts", k, (long)n_sq, (long)n_q);
            // { offset, bytes the kernels index }
            std::vector<std::pair<size_t, size_t>> r = {
                {c.queries, 32 * n_q}, {c.words, 4 * c.lanes},     {c.bsum, 32 * c.blocks}, {c.csum, 32 * c.chunks},
                {c.totals, 32},        {c.per, 4 * c.pairs},       {c.req, 16 * cap},       {c.node_off, 8 * (cap + 1)},
                {c.leaf_off, 8 * (cap + 1)}, {c.abs_rec, 8 * cap}, {c.hits, 8 * cap}};
            for (const auto& x : r)
              if (x.first % 256 || x.first + x.second > c.total) return fail("carve region", k, (long)x.first);
            std::sort(r.begin(), r.end());
            for (size_t i = 1; i < r.size(); i++)
              if (r[i - 1].first + r[i - 1].second > r[i].first) return fail("carve overlap", k, (long)i);
            // at most 4 B per lane beyond the per-block, per-pair and per-proof parts
            if (c.total > 4 * c.lanes + 32 * (c.blocks + c.chunks) + 4 * c.pairs + 32 * n_q + 48 * cap + 13 * 256)
              return fail("carve size", k, (long)c.total);
            if (c.total < prev_cap) return fail("carve not monotone in proofs_cap", k);
            prev_cap = c.total;
            if (cap == caps[0]) {
              if (c.total < prev_q) return fail("carve not monotone in n_q", k);
              prev_q = c.total;
              if (n_q == nqs[1]) {
                if (c.total < prev_sq) return fail("carve not monotone in n_sq", k);
                prev_sq = c.total;
              }
            }
            carves++;
          }
        }
      }
    }
    NsSqCarve c;
    if (ns_squares_carve(8, 0, 4, 0, &c)) return fail("no squares accepted");
    if (ns_squares_carve(128, 1u << 20, 1u << 20, 0, &c)) return fail("overflow accepted");
    if (ns_squares_carve(1, 1, ((size_t)1 << 30), 0, &c)) return fail("2^31 lanes accepted");
    if (!ns_squares_carve(1, 1, ((size_t)1 << 30) - 128, 0, &c)) return fail("largest batch refused");
    if (ns_squares_carve(128, ~(size_t)0 / 2, 3, 0, &c)) return fail("wrapping product accepted");
    rejected += 4;
  }

  printf("ok words=%ld tables=%ld proofs=%ld rejected=%ld carves=%ld\n", words, tables, proofs, rejected, carves);
  return 0;
}
