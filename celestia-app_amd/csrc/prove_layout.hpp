// prove_layout.hpp -- request checks, output layout and the node rule of the
// batched range-proof producer (dagpu_nmt_prove_batch_device, nmt_prove.hip).
// Host arithmetic only (no HIP include), so that tests/host/prove_layout_check.cpp
// can compile it without a GPU; the one function the emit kernel shares
// (prove_node_at) is marked for both sides when hipcc compiles it.
//
// nmt ProveRange(start, end) on a full tree of w = 2^m leaves emits the roots of
// the maximal subtrees disjoint from [start, end), left to right
// (buildRangeProof; celestia_da/proof.py range_proof_nodes is the
// specification).  In closed form:
//   * left of the range, for each set bit b of start from high to low: the
//     node at depth m - b, position (start >> b) - 1;
//   * right of it, for each zero bit b of end - 1 from b = 0 up to m - 1: the
//     node at depth m - b, position ((end - 1) >> b) + 1;
//   * popcount(start) + m - popcount(end - 1) nodes in all (none for [0, w)).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define DAGPU_PROVE_HD __host__ __device__
#else
#define DAGPU_PROVE_HD
#endif

namespace dagpu {

constexpr int kProveReqWords = 4;   // int64 per request: axis, index, start, end (dagpu.h DAGPU_PROVE_REQ_WORDS)
constexpr int kProveDescWords = 8;  // int64 per descriptor written (dagpu.h DAGPU_NMT_DESC_WORDS)

DAGPU_PROVE_HD inline int prove_popcount(uint32_t v) {
  int c = 0;
  for (; v; v &= v - 1) c++;
  return c;
}

// nodes of ProveRange(start, end) in a tree of 2^m leaves, 0 <= start < end <= 2^m
DAGPU_PROVE_HD inline int prove_node_count(int m, uint32_t start, uint32_t end) {
  return prove_popcount(start) + m - prove_popcount(end - 1);
}

// node j (0 <= j < prove_node_count) of that proof: depth (0 = root) and
// position within its level
DAGPU_PROVE_HD inline void prove_node_at(int m, uint32_t start, uint32_t end, int j, int* depth, uint32_t* pos) {
  for (int b = m - 1; b >= 0; b--) {  // left of the range, widest subtree first
    if (!((start >> b) & 1u)) continue;
    if (j == 0) {
      *depth = m - b;
      *pos = (start >> b) - 1;
      return;
    }
    j--;
  }
  const uint32_t last = end - 1;
  for (int b = 0; b < m; b++) {  // right of the range, narrowest subtree first
    if ((last >> b) & 1u) continue;
    if (j == 0) {
      *depth = m - b;
      *pos = (last >> b) + 1;
      return;
    }
    j--;
  }
  *depth = 0;  // not reached for j < prove_node_count
  *pos = 0;
}

// Why a batch was refused (prove_layout); kProveOk otherwise.
enum ProveCheck {
  kProveOk = 0,
  kProveBadAxis,    // axis not 0 or 1
  kProveBadIndex,   // index outside [0, 2k)
  kProveBadRange,   // not 0 <= start < end <= 2k
  kProveNoColumns,  // an axis-1 request without the column inner levels
  kProveNodesCap,   // more nodes than nodes_cap
  kProveSharesCap,  // more proven cells than shares_cap
};

// Where every proof's nodes and cells go: node_off / leaf_off are prefix sums
// over the requests in order (n + 1 entries each), packed with no gaps.
struct ProveLayout {
  std::vector<int64_t> node_off, leaf_off;
  int64_t n_nodes = 0, n_leaves = 0;
};

inline int prove_log2(uint32_t w) {
  int m = 0;
  while ((1u << m) < w) m++;
  return m;
}

// Check every request of the batch (k a power of two) and lay the outputs
// out.  check_shares: shares are wanted, so the cell total must fit
// shares_cap.  On a refusal *bad is the first offending request (n for a
// capacity) and `out` holds nothing to use.
inline ProveCheck prove_layout(uint32_t k, size_t n, const int64_t* req, bool have_columns, size_t nodes_cap,
                               bool check_shares, size_t shares_cap, ProveLayout* out, size_t* bad) {
  const int64_t w = 2 * (int64_t)k;
  const int m = prove_log2((uint32_t)w);
  out->node_off.assign(n + 1, 0);
  out->leaf_off.assign(n + 1, 0);
  int64_t nodes = 0, leaves = 0;
  for (size_t i = 0; i < n; i++) {
    const int64_t* r = req + i * kProveReqWords;
    const int64_t axis = r[0], index = r[1], start = r[2], end = r[3];
    *bad = i;
    if (axis != 0 && axis != 1) return kProveBadAxis;
    if (index < 0 || index >= w) return kProveBadIndex;
    if (start < 0 || start >= end || end > w) return kProveBadRange;
    if (axis == 1 && !have_columns) return kProveNoColumns;
    out->node_off[i] = nodes;
    out->leaf_off[i] = leaves;
    nodes += prove_node_count(m, (uint32_t)start, (uint32_t)end);
    leaves += end - start;
  }
  *bad = n;
  out->node_off[n] = out->n_nodes = nodes;
  out->leaf_off[n] = out->n_leaves = leaves;
  if ((uint64_t)nodes > (uint64_t)nodes_cap) return kProveNodesCap;
  if (check_shares && (uint64_t)leaves > (uint64_t)shares_cap) return kProveSharesCap;
  return kProveOk;
}

// Descriptors of dagpu_nmt_verify_batch(_device) for the produced proofs:
// {start, end, n_leaves, leaf_off, n_nodes, node_off, ns_index, root_index},
// leaves in the producer's packed share output, namespace i of its namespace
// output, roots in a table row_roots || col_roots (4k x 90 B).
inline void prove_fill_desc(uint32_t k, size_t n, const int64_t* req, const ProveLayout& lay, int64_t* desc) {
  for (size_t i = 0; i < n; i++) {
    const int64_t* r = req + i * kProveReqWords;
    int64_t* d = desc + i * kProveDescWords;
    d[0] = r[2];
    d[1] = r[3];
    d[2] = r[3] - r[2];
    d[3] = lay.leaf_off[i];
    d[4] = lay.node_off[i + 1] - lay.node_off[i];
    d[5] = lay.node_off[i];
    d[6] = (int64_t)i;
    d[7] = r[0] * 2 * (int64_t)k + r[1];
  }
}

// One validated request as the kernels read it: four uint16 in one 8-B word
// (index < 2k <= 16384 and end <= 2k fit).
inline uint64_t prove_pack_req(const int64_t* r) {
  return (uint64_t)r[0] | ((uint64_t)r[1] << 16) | ((uint64_t)r[2] << 32) | ((uint64_t)r[3] << 48);
}

}  // namespace dagpu
