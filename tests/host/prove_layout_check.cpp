// Stand-alone host check of csrc/prove_layout.hpp (tests/test_prove_layout_host.py
// compiles and runs it; no GPU, no HIP).
//   * For every tree of 1, 2, 4 .. 128 leaves and every range [start, end):
//     prove_node_count and the (depth, position) list of prove_node_at equal
//     nmt's recursive buildRangeProof, restated here.
//   * A batch of every (axis, index, range) of a k = 4 square: node_off and
//     leaf_off are the prefix sums, the descriptors have the verifier's
//     format, and the packed request words unpack to the request.
//   * Each invalid request class and each capacity one too small is refused
//     with its own reason, naming the offending request.
#include <stdint.h>
#include <stdio.h>

#include <utility>
#include <vector>

#include "../../celestia-app_amd/csrc/prove_layout.hpp"

using namespace dagpu;

// nmt buildRangeProof on a full tree: a subtree disjoint from [start, end) is
// emitted whole, a leaf inside the range emits nothing, anything else recurses
// left then right.
static void build_range_proof(int64_t lo, int64_t hi, int depth, int max_depth, int64_t start, int64_t end,
                              std::vector<std::pair<int, int64_t>>* out) {
  if (hi <= start || lo >= end) {
    out->push_back({depth, lo >> (max_depth - depth)});
    return;
  }
  if (hi - lo == 1) return;
  const int64_t mid = (lo + hi) / 2;
  build_range_proof(lo, mid, depth + 1, max_depth, start, end, out);
  build_range_proof(mid, hi, depth + 1, max_depth, start, end, out);
}

static int fail(const char* what, long a = 0, long b = 0, long c = 0) {
  printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
  return 1;
}

int main() {
  long ranges = 0, nodes = 0;
  for (int m = 0; m <= 7; m++) {
    const int64_t w = (int64_t)1 << m;
    if (prove_log2((uint32_t)w) != m) return fail("prove_log2", m);
    for (int64_t s = 0; s < w; s++)
      for (int64_t e = s + 1; e <= w; e++) {
        std::vector<std::pair<int, int64_t>> want;
        build_range_proof(0, w, 0, m, s, e, &want);
        const int cnt = prove_node_count(m, (uint32_t)s, (uint32_t)e);
        if (cnt != (int)want.size()) return fail("count", w, s, e);
        for (int j = 0; j < cnt; j++) {
          int depth = -1;
          uint32_t pos = ~0u;
          prove_node_at(m, (uint32_t)s, (uint32_t)e, j, &depth, &pos);
          if (depth != want[j].first || (int64_t)pos != want[j].second) return fail("node", w, s, e);
          if (depth < 1 || depth > m || pos >= (1u << depth)) return fail("node outside the tree", w, s, e);
        }
        ranges++;
        nodes += cnt;
      }
  }

  // one batch: every request of a k = 4 square, axes interleaved
  const uint32_t k = 4;
  const int64_t w = 2 * k;
  std::vector<int64_t> req;
  for (int64_t index = 0; index < w; index++)
    for (int64_t s = 0; s < w; s++)
      for (int64_t e = s + 1; e <= w; e++)
        for (int64_t axis = 0; axis < 2; axis++) {
          const int64_t r[4] = {axis, index, s, e};
          req.insert(req.end(), r, r + 4);
        }
  const size_t n = req.size() / 4;
  ProveLayout lay;
  size_t bad = 0;
  if (prove_layout(k, n, req.data(), true, (size_t)1 << 40, true, (size_t)1 << 40, &lay, &bad) != kProveOk)
    return fail("valid batch refused", (long)bad);
  if (lay.node_off.size() != n + 1 || lay.leaf_off.size() != n + 1) return fail("offset array sizes");
  std::vector<int64_t> desc(n * kProveDescWords, -7);
  prove_fill_desc(k, n, req.data(), lay, desc.data());
  int64_t no = 0, lo = 0;
  for (size_t i = 0; i < n; i++) {
    const int64_t* r = &req[4 * i];
    const int cnt = prove_node_count(3, (uint32_t)r[2], (uint32_t)r[3]);
    if (lay.node_off[i] != no || lay.leaf_off[i] != lo) return fail("prefix sum", (long)i);
    const int64_t want[8] = {r[2], r[3], r[3] - r[2], lo, cnt, no, (int64_t)i, r[0] * w + r[1]};
    for (int j = 0; j < 8; j++)
      if (desc[8 * i + j] != want[j]) return fail("descriptor", (long)i, j);
    const uint64_t p = prove_pack_req(r);
    if ((int64_t)(p & 0xFFFF) != r[0] || (int64_t)((p >> 16) & 0xFFFF) != r[1] ||
        (int64_t)((p >> 32) & 0xFFFF) != r[2] || (int64_t)(p >> 48) != r[3])
      return fail("packed request", (long)i);
    no += cnt;
    lo += r[3] - r[2];
  }
  if (lay.node_off[n] != no || lay.n_nodes != no || lay.leaf_off[n] != lo || lay.n_leaves != lo)
    return fail("totals");
  // the widest square: end = 2k = 16384 still fits a packed request
  {
    const int64_t r[4] = {1, 16383, 16383, 16384};
    const uint64_t p = prove_pack_req(r);
    if ((p & 0xFFFF) != 1 || ((p >> 16) & 0xFFFF) != 16383 || ((p >> 32) & 0xFFFF) != 16383 || (p >> 48) != 16384)
      return fail("packed request at k = 8192");
  }

  // capacities: exact fits, one too small does not; shares only when wanted
  if (prove_layout(k, n, req.data(), true, (size_t)no, true, (size_t)lo, &lay, &bad) != kProveOk)
    return fail("exact capacities refused");
  if (prove_layout(k, n, req.data(), true, (size_t)no - 1, true, (size_t)lo, &lay, &bad) != kProveNodesCap || bad != n)
    return fail("nodes_cap - 1 accepted");
  if (prove_layout(k, n, req.data(), true, (size_t)no, true, (size_t)lo - 1, &lay, &bad) != kProveSharesCap || bad != n)
    return fail("shares_cap - 1 accepted");
  if (prove_layout(k, n, req.data(), true, (size_t)no, false, 0, &lay, &bad) != kProveOk)
    return fail("shares_cap checked though no shares are wanted");

  // invalid request classes, each at position 5 of a small valid batch
  struct Case {
    int64_t r[4];
    bool have_columns;
    ProveCheck want;
  };
  const Case cases[] = {
      {{2, 0, 0, 1}, true, kProveBadAxis},      {{-1, 0, 0, 1}, true, kProveBadAxis},
      {{0, -1, 0, 1}, true, kProveBadIndex},    {{0, w, 0, 1}, true, kProveBadIndex},
      {{1, w, 0, 1}, true, kProveBadIndex},     {{0, 0, -1, 1}, true, kProveBadRange},
      {{0, 0, 3, 3}, true, kProveBadRange},     {{0, 0, 4, 3}, true, kProveBadRange},
      {{0, 0, 0, w + 1}, true, kProveBadRange}, {{0, 0, w, w + 1}, true, kProveBadRange},
      {{0, 0, 0, 0}, true, kProveBadRange},     {{1, 0, 0, 1}, false, kProveNoColumns},
      {{0, 0, 0, (int64_t)1 << 40}, true, kProveBadRange},
      {{0, (int64_t)1 << 40, 0, 1}, true, kProveBadIndex},
      {{(int64_t)1 << 32, 0, 0, 1}, true, kProveBadAxis},
  };
  long refused = 0;
  for (const Case& c : cases) {
    std::vector<int64_t> b;
    for (int i = 0; i < 8; i++) {
      const int64_t ok[4] = {0, i, 0, w};
      b.insert(b.end(), ok, ok + 4);
    }
    for (int j = 0; j < 4; j++) b[4 * 5 + j] = c.r[j];
    if (prove_layout(k, 8, b.data(), c.have_columns, 1000, true, 1000, &lay, &bad) != c.want || bad != 5)
      return fail("invalid request accepted or misreported", c.r[0], c.r[1], c.r[2]);
    refused++;
  }
  // without the column levels, row requests alone are fine
  {
    const int64_t ok[4] = {0, 1, 2, 3};
    if (prove_layout(k, 1, ok, false, 10, true, 10, &lay, &bad) != kProveOk) return fail("row request refused");
  }
  printf("ok ranges=%ld nodes=%ld batch=%zu refused=%ld\n", ranges, nodes, n, refused);
  return 0;
}
