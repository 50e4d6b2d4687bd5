// prove_host.cpp -- host side of the proof producer (include/dagpu.h): request
// checks, layout, uploads and launches.  The kernels check nothing.
//   dagpu_nmt_prove_batch_device   nmt ProveRange for many requests on the row and
//       column trees of a resident square (pkg/proof/proof.go:87-150): nodes selected
//       on the device (nmt_prove.hip), checks and layout in prove_layout.hpp
//   dagpu_proof_store_device / dagpu_nmt_prove_squares_device / dagpu_share_proof_requests
//       the same for all n squares of a batch and on to the data root (RowProof,
//       proof.go:84-91): one store built with a launch count independent of n
//       (proof_store.hip); layout and the row split in share_proof_layout.hpp
//   dagpu_nmt_namespace_ranges_device / dagpu_nmt_prove_namespace_batch_device
//       nmt ProveNamespace on every row tree of a resident square: search on the
//       device (nmt_namespace.hip, ns_find.hpp), then the emit and gather kernels
//   dagpu_nmt_namespace_squares_count_device / dagpu_nmt_prove_namespace_squares_device
//       the same across a batch proof store: hits counted, ordered and laid out on
//       the device (ns_squares_layout.hpp); only the hit records come back
// All four producers fill one ProveArgs (forest.hpp) and launch by prove_launch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/dagpu.h"
#include "forest.hpp"
#include "ns_find.hpp"
#include "ns_squares_layout.hpp"
#include "pipe_carve.hpp"
#include "proof_verify.hpp"
#include "prove_layout.hpp"
#include "runtime.hpp"
#include "share_proof_layout.hpp"

namespace {

// what every entry point here asks first: a context and a supported width
int check_ctx_k(dagpu_ctx* ctx, uint32_t k) { return ctx ? check_k(ctx, k) : DAGPU_ERR_ARG; }

// The stores of a call, square i's part of each at base + i * its size in l:
// the regions of a batch proof store, or the two exports of one square (no
// DAH tree, l and square_stride 0: no request names a square).
ProveArgs prove_args(uint32_t k, const uint8_t* d_rows, const uint8_t* d_cols, const uint8_t* d_dah,
                     const ProofStoreLayout& l, const uint8_t* d_eds, size_t square_stride) {
  ProveArgs a{};
  a.w = 2 * (int)k;
  a.logw = prove_log2(2 * k);
  a.row_nodes = d_rows;
  a.col_inner = d_cols;
  a.dah = d_dah;
  a.eds = d_eds;
  a.row_bytes = (long)l.row_bytes;
  a.col_bytes = (long)l.col_bytes;
  a.dah_bytes = (long)l.dah_bytes;
  a.square_stride = (long)square_stride;
  return a;
}

// The tables of n proofs with requests of `words` 8-B words each.
void prove_tables(ProveArgs* a, int words, size_t n, const int64_t* req, const int64_t* node_off,
                  const int64_t* leaf_off, int64_t n_nodes, int64_t n_leaves) {
  a->n = (long)n;
  a->req_words = words;
  a->req = req;
  a->node_off = node_off;
  a->leaf_off = leaf_off;
  a->n_nodes = (long)n_nodes;
  a->n_leaves = (long)n_leaves;
}

// Every output a names: the nmt proofs, then what else was asked for.
int prove_launch(dagpu_ctx* ctx, const ProveArgs& a, hipStream_t s) {
  HIP_TRY(ctx, launch_prove_emit(a, s));
  if (a.ns_out) HIP_TRY(ctx, launch_prove_namespaces(a, s));
  if (a.shares_out) HIP_TRY(ctx, launch_prove_shares(a, s));
  if (a.axis_roots_out || a.leaf_hash_out || a.aunts_out) HIP_TRY(ctx, launch_prove_sq_merkle(a, s));
  return DAGPU_OK;
}

// Build the image requests | node_off (n + 1) | leaf_off (n + 1) from validated
// requests (words == 1: 4-word requests, 2: 5-word requests with the square
// first) and their layout, upload it to d_ws and wait (the image and the
// caller's requests may go), then launch for the outputs a names.
int prove_requests(dagpu_ctx* ctx, ProveArgs* a, int words, size_t n, const int64_t* req, const ProveLayout& lay,
                   void* d_ws, hipStream_t s) {
  std::vector<int64_t> meta((words + 2) * n + 2);
  for (size_t i = 0; i < n; i++) {
    if (words == 1) meta[i] = (int64_t)prove_pack_req(req + i * kProveReqWords);
    else prove_squares_pack_req(req + i * kProveSqReqWords, &meta[2 * i]);
  }
  memcpy(meta.data() + words * n, lay.node_off.data(), (n + 1) * sizeof(int64_t));
  memcpy(meta.data() + (words + 1) * n + 1, lay.leaf_off.data(), (n + 1) * sizeof(int64_t));
  HIP_TRY(ctx, hipMemcpyAsync(d_ws, meta.data(), meta.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  const int64_t* t = (const int64_t*)d_ws;
  prove_tables(a, words, n, t, t + words * n, t + (words + 1) * n + 1, lay.n_nodes, lay.n_leaves);
  return prove_launch(ctx, *a, s);
}

// What prove_layout / prove_squares_layout refused, as the caller reads it.
int prove_refusal(dagpu_ctx* ctx, int pc, size_t bad, size_t n) {
  const char* why = pc == kProveBadSquare    ? "square outside the batch"
                    : pc == kProveBadAxis    ? "axis is not 0 or 1"
                    : pc == kProveBadIndex   ? "index outside the square"
                    : pc == kProveBadRange   ? "range is not 0 <= start < end <= 2k"
                    : pc == kProveNoColumns  ? "column request without column nodes"
                    : pc == kProveNodesCap   ? "more proof nodes than nodes_cap"
                                             : "more proven cells than shares_cap";
  return set_err(ctx, DAGPU_ERR_ARG,
                 (bad < n ? "proof request " + std::to_string(bad) + ": " : std::string("proof batch: ")) + why);
}

// ---- helpers of the namespace calls ----

// no proof at all (and what a call without queries returns)
int ns_zero_counts(int64_t* counts) {
  if (counts) counts[0] = counts[1] = counts[2] = counts[3] = 0;
  return DAGPU_OK;
}

// The query namespaces zero padded to 32 B each, and their upload to d.
// `padded` is read by the upload: it must outlive the next synchronisation.
hipError_t ns_upload_queries(std::vector<uint8_t>* padded, size_t n_q, const uint8_t* namespaces, uint8_t* d,
                             hipStream_t s) {
  padded->assign(32 * n_q, 0);
  for (size_t q = 0; q < n_q; q++) memcpy(padded->data() + 32 * q, namespaces + q * kNsSize, kNsSize);
  return hipMemcpyAsync(d, padded->data(), padded->size(), hipMemcpyHostToDevice, s);
}

// The search needs more room than the caller gave: refuse, naming the needs.
int ns_check_capacity(dagpu_ctx* ctx, const std::string& who, const int64_t need[4], size_t proofs_cap,
                      size_t leaf_hashes_cap, size_t nodes_cap, size_t shares_cap) {
  if (ns_sq_short_capacity(need, proofs_cap, leaf_hashes_cap, nodes_cap, shares_cap) < 0) return DAGPU_OK;
  return set_err(ctx, DAGPU_ERR_ARG, who + ": a capacity is too small (proofs " + std::to_string(need[0]) +
                                         ", leaf hashes " + std::to_string(need[1]) + ", nodes " +
                                         std::to_string(need[2]) + ", cells " + std::to_string(need[3]) + " needed)");
}

// Search every (query, row) on the device and read the ranges back: one
// synchronisation.  `ranges` gets n_q * 2k triples; counts as dagpu.h states.
int ns_search(dagpu_ctx* ctx, uint32_t k, size_t n_q, const uint8_t* namespaces, const uint8_t* d_row_nodes,
              int32_t* ranges, int64_t counts[4], uint8_t* d_ws, hipStream_t s) {
  const size_t w = 2 * (size_t)k, pairs = n_q * w;
  const int m = prove_log2((uint32_t)w);
  std::vector<uint8_t> padded;
  int32_t* d_ranges = (int32_t*)(d_ws + ws_align256(32 * n_q));
  HIP_TRY(ctx, ns_upload_queries(&padded, n_q, namespaces, d_ws, s));
  NsFindArgs a{};
  a.n_q = (long)n_q;
  a.w = (int)w;
  a.queries = d_ws;
  a.row_nodes = d_row_nodes;
  a.ranges = d_ranges;
  hipError_t e = launch_ns_find(a, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(ranges, d_ranges, pairs * kNsRangeWords * sizeof(int32_t), hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);  // `padded` is read by the upload: always wait
  HIP_TRY(ctx, e);
  HIP_TRY(ctx, e2);
  (void)ns_zero_counts(counts);
  for (size_t p = 0; p < pairs; p++) {
    const int32_t* r = ranges + p * kNsRangeWords;
    // what the kernel wrote is re-checked before anything is laid out from it
    if (r[0] < kNsOutside || r[0] > kNsAbsent || (r[0] != kNsOutside && !(0 <= r[1] && r[1] < r[2] && r[2] <= (int32_t)w)))
      return set_err(ctx, DAGPU_ERR_DEVICE, "namespace search returned a range outside the row");
    if (r[0] == kNsOutside) continue;
    counts[0]++;
    counts[2] += prove_node_count(m, (uint32_t)r[1], (uint32_t)r[2]);
    if (r[0] == kNsAbsent) counts[1]++; else counts[3] += r[2] - r[1];
  }
  return DAGPU_OK;
}

// d_nodes: the row store, or the batch proof store
int ns_common_check(dagpu_ctx* ctx, const std::string& who, const void* namespaces, const void* d_nodes,
                    const void* d_workspace) {
  if (!namespaces || !d_nodes || !d_workspace) return set_err(ctx, DAGPU_ERR_ARG, who + ": null buffer");
  if ((((uintptr_t)d_workspace | (uintptr_t)d_nodes) & 15) != 0)
    return set_err(ctx, DAGPU_ERR_ARG, who + ": misaligned buffer");
  return DAGPU_OK;
}

// Upload the padded queries, search every (query, square, row), count and scan
// on the device and read the four totals (and per_out) back: one
// synchronisation.  `a` is left ready for the scatter.
int ns_sq_search(dagpu_ctx* ctx, uint32_t k, size_t n_sq, size_t n_q, const uint8_t* namespaces,
                 const uint8_t* d_store, const NsSqCarve& c, size_t row_bytes, int64_t totals[4], int32_t* per_out,
                 uint8_t* ws, hipStream_t s, NsSqArgs* args) {
  NsSqArgs& a = *args = NsSqArgs{};
  a.n_q = (long)n_q;
  a.n_sq = (long)n_sq;
  a.w = (int)(2 * k);
  a.logw = prove_log2(2 * k);
  a.lanes = (long)c.lanes;
  a.pairs = (long)c.pairs;
  a.blocks = (long)c.blocks;
  a.chunks = (long)c.chunks;
  a.queries = ws + c.queries;
  a.store = d_store;
  a.row_bytes = (long)row_bytes;
  a.words = (uint32_t*)(ws + c.words);
  a.bsum = (int64_t*)(ws + c.bsum);
  a.csum = (int64_t*)(ws + c.csum);
  a.totals = (int64_t*)(ws + c.totals);
  a.per = per_out ? (int32_t*)(ws + c.per) : nullptr;
  a.req = (int64_t*)(ws + c.req);
  a.node_off = (int64_t*)(ws + c.node_off);
  a.leaf_off = (int64_t*)(ws + c.leaf_off);
  a.abs_rec = (int64_t*)(ws + c.abs_rec);
  a.hits = (uint32_t*)(ws + c.hits);
  int64_t got[kNsSqSums];
  std::vector<uint8_t> padded;
  std::vector<int32_t> per(per_out ? c.pairs : 0);
  hipError_t e = ns_upload_queries(&padded, n_q, namespaces, ws + c.queries, s);
  if (e == hipSuccess) e = launch_ns_sq_search(a, s);
  if (e == hipSuccess) e = hipMemcpyAsync(got, a.totals, sizeof got, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && per_out)
    e = hipMemcpyAsync(per.data(), a.per, per.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);  // `padded` is read by the upload: always wait
  HIP_TRY(ctx, e);
  HIP_TRY(ctx, e2);
  // what the device reports is checked before anything is sized from it
  bool ok = ns_sq_totals_ok(got, c.lanes, a.logw, (uint32_t)a.w);
  int64_t per_sum = 0;
  for (size_t i = 0; ok && i < per.size(); i++) {
    ok = per[i] >= 0 && per[i] <= a.w;
    per_sum += per[i];
  }
  if (!ok || (per_out && per_sum != got[0]))
    return set_err(ctx, DAGPU_ERR_DEVICE, "namespace search returned counts outside the batch");
  memcpy(totals, got, sizeof got);
  if (per_out) memcpy(per_out, per.data(), per.size() * sizeof(int32_t));
  return DAGPU_OK;
}

int ns_sq_common_check(dagpu_ctx* ctx, const std::string& who, uint32_t k, size_t n_sq, size_t n_q, size_t proofs_cap,
                       const void* namespaces, const void* d_store, const void* d_workspace, NsSqCarve* c,
                       ProofStoreLayout* l) {
  if (!proof_store_layout(k, n_sq, l) || !ns_squares_carve(k, n_sq, n_q, proofs_cap, c))
    return set_err(ctx, DAGPU_ERR_ARG, who + ": the (query, square, row) count or a size overflows");
  return ns_common_check(ctx, who, namespaces, d_store, d_workspace);
}

}  // namespace

extern "C" {

// ---- range proofs from one resident square and from a batch proof store (nmt_prove.hip) ----

size_t dagpu_nmt_prove_workspace_size(size_t n) {
  // packed requests (n) | node_off (n + 1) | leaf_off (n + 1), 8 B each
  return ws_align256((3 * n + 2) * sizeof(int64_t)) + 256;
}

int dagpu_nmt_prove_batch_device(dagpu_ctx* ctx, uint32_t k, size_t n, const int64_t* req, const uint8_t* d_eds,
                                 const uint8_t* d_row_nodes, const uint8_t* d_col_inner, uint8_t* d_nodes_out,
                                 size_t nodes_cap, uint8_t* d_ns_out, uint8_t* d_shares_out, size_t shares_cap,
                                 int64_t* desc_out, size_t* n_nodes_total, void* d_workspace, void* stream) {
  int rc = check_ctx_k(ctx, k);
  if (rc) return rc;
  if (n == 0) {
    if (n_nodes_total) *n_nodes_total = 0;
    return DAGPU_OK;
  }
  if (!req || !d_row_nodes || !d_workspace || (nodes_cap && !d_nodes_out) || (d_shares_out && !d_eds))
    return set_err(ctx, DAGPU_ERR_ARG, "dagpu_nmt_prove_batch_device: null buffer");
  if ((((uintptr_t)d_workspace | (uintptr_t)d_row_nodes | (uintptr_t)d_col_inner | (uintptr_t)d_eds |
        (uintptr_t)d_shares_out) & 15) != 0 || (((uintptr_t)d_nodes_out) & 1) != 0)
    return set_err(ctx, DAGPU_ERR_ARG, "dagpu_nmt_prove_batch_device: misaligned buffer");
  ProveLayout lay;
  size_t bad = 0;
  const ProveCheck pc = prove_layout(k, n, req, d_col_inner != nullptr, nodes_cap, d_shares_out != nullptr,
                                     shares_cap, &lay, &bad);
  if (pc != kProveOk) return prove_refusal(ctx, pc, bad, n);
  hipStream_t s = (hipStream_t)stream;
  ProveArgs a = prove_args(k, d_row_nodes, d_col_inner, nullptr, ProofStoreLayout{}, d_eds, 0);
  a.nodes_out = d_nodes_out;
  a.ns_out = d_ns_out;
  a.shares_out = d_shares_out;
  rc = prove_requests(ctx, &a, 1, n, req, lay, d_workspace, s);
  if (rc) return rc;
  if (desc_out) prove_fill_desc(k, n, req, lay, desc_out);
  if (n_nodes_total) *n_nodes_total = (size_t)lay.n_nodes;
  return DAGPU_OK;
}

size_t dagpu_proof_store_size(uint32_t k, size_t n, size_t* col_off, size_t* dah_off) {
  ProofStoreLayout l;
  if (k == 0 || !is_pow2(k) || k > (uint32_t)kMaxK || n == 0 || !proof_store_layout(k, n, &l)) return 0;
  if (col_off) *col_off = l.col_off;
  if (dah_off) *dah_off = l.dah_off;
  return l.total;
}

size_t dagpu_proof_store_workspace_size(uint32_t k, size_t n) {
  if (dagpu_proof_store_size(k, n, nullptr, nullptr) == 0) return 0;
  return 256;  // the shapes are uniform: nothing is uploaded, the workspace is reserved
}

int dagpu_proof_store_device(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* d_eds, size_t square_stride,
                             uint8_t* d_store, void* d_workspace, void* stream) {
  int rc = check_ctx_k(ctx, k);
  if (rc) return rc;
  ProofStoreLayout l;
  if (n == 0 || !proof_store_layout(k, n, &l))
    return set_err(ctx, DAGPU_ERR_ARG, "dagpu_proof_store_device: no squares, or a store beyond the address space");
  if (!d_eds || !d_store || !d_workspace)
    return set_err(ctx, DAGPU_ERR_ARG, "dagpu_proof_store_device: null buffer");
  const size_t w = 2 * (size_t)k;
  if ((((uintptr_t)d_eds | (uintptr_t)d_store | square_stride) & 15) != 0 || square_stride < w * w * kShareSize)
    return set_err(ctx, DAGPU_ERR_ARG,
                   "dagpu_proof_store_device: buffers and square_stride must be multiples of 16 B, squares must "
                   "not overlap");
  ProofStoreArgs a{};
  a.n = (long)n;
  a.k = (int)k;
  a.w = (int)w;
  a.logw = prove_log2((uint32_t)w);
  a.eds = d_eds;
  a.square_stride = (long)square_stride;
  a.store = d_store;
  a.row_bytes = (long)l.row_bytes;
  a.col_bytes = (long)l.col_bytes;
  a.dah_bytes = (long)l.dah_bytes;
  a.col_off = (long)l.col_off;
  a.dah_off = (long)l.dah_off;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(ctx, launch_store_leaves(a, s));
  for (int L = 1; L <= a.logw; L++) HIP_TRY(ctx, launch_store_level(a, L, s));
  for (int L = 0; L <= a.logw + 1; L++) HIP_TRY(ctx, launch_store_dah_level(a, L, s));
  return DAGPU_OK;
}

size_t dagpu_nmt_prove_squares_workspace_size(size_t n_req) {
  // requests (2 words each) | node_off (n + 1) | leaf_off (n + 1), 8 B each
  return ws_align256((4 * n_req + 2) * sizeof(int64_t)) + 256;
}

int dagpu_nmt_prove_squares_device(dagpu_ctx* ctx, uint32_t k, size_t n_sq, size_t n_req, const int64_t* req,
                                   const uint8_t* d_eds, size_t square_stride, const uint8_t* d_store,
                                   uint8_t* d_nodes_out, size_t nodes_cap, uint8_t* d_ns_out, uint8_t* d_shares_out,
                                   size_t shares_cap, uint8_t* d_axis_roots_out, uint8_t* d_leaf_hash_out,
                                   uint8_t* d_aunts_out, int64_t* desc_out, int64_t* mdesc_out,
                                   size_t* n_nodes_total, void* d_workspace, void* stream) {
  int rc = check_ctx_k(ctx, k);
  if (rc) return rc;
  if (n_req == 0) {
    if (n_nodes_total) *n_nodes_total = 0;
    return DAGPU_OK;
  }
  ProofStoreLayout l;
  if (n_sq == 0 || !proof_store_layout(k, n_sq, &l))
    return set_err(ctx, DAGPU_ERR_ARG, "dagpu_nmt_prove_squares_device: no squares");
  if (!req || !d_store || !d_workspace || (nodes_cap && !d_nodes_out) || (d_shares_out && !d_eds))
    return set_err(ctx, DAGPU_ERR_ARG, "dagpu_nmt_prove_squares_device: null buffer");
  if ((((uintptr_t)d_workspace | (uintptr_t)d_store | (uintptr_t)d_eds | (uintptr_t)d_shares_out |
        (uintptr_t)d_leaf_hash_out | (uintptr_t)d_aunts_out | (d_shares_out ? square_stride : 0)) & 15) != 0 ||
      ((((uintptr_t)d_nodes_out) | (uintptr_t)d_axis_roots_out) & 1) != 0)
    return set_err(ctx, DAGPU_ERR_ARG, "dagpu_nmt_prove_squares_device: misaligned buffer");
  const size_t w = 2 * (size_t)k;
  if (d_shares_out && square_stride < w * w * kShareSize)
    return set_err(ctx, DAGPU_ERR_ARG, "dagpu_nmt_prove_squares_device: square_stride smaller than a square");
  ProveLayout lay;
  size_t bad = 0;
  const int pc = prove_squares_layout(k, n_sq, n_req, req, nodes_cap, d_shares_out != nullptr, shares_cap, &lay, &bad);
  if (pc != kProveOk) return prove_refusal(ctx, pc, bad, n_req);
  hipStream_t s = (hipStream_t)stream;
  ProveArgs a = prove_args(k, d_store, d_store + l.col_off, d_store + l.dah_off, l, d_eds, square_stride);
  a.nodes_out = d_nodes_out;
  a.ns_out = d_ns_out;
  a.shares_out = d_shares_out;
  a.axis_roots_out = d_axis_roots_out;
  a.leaf_hash_out = d_leaf_hash_out;
  a.aunts_out = d_aunts_out;
  rc = prove_requests(ctx, &a, 2, n_req, req, lay, d_workspace, s);
  if (rc) return rc;
  if (desc_out) prove_squares_fill_desc(n_req, req, lay, desc_out);
  if (mdesc_out) prove_squares_fill_mdesc(k, n_req, req, mdesc_out);
  if (n_nodes_total) *n_nodes_total = (size_t)lay.n_nodes;
  return DAGPU_OK;
}

int dagpu_share_proof_requests(uint32_t k, size_t n_sq, size_t n, const int64_t* sreq, int64_t* req_out, size_t cap,
                               int64_t* span_out, size_t* n_req) {
  if (k == 0 || !is_pow2(k) || k > (uint32_t)kMaxK || (n && (!sreq || !req_out))) return DAGPU_ERR_ARG;
  return share_proof_requests(k, n_sq, n, sreq, req_out, cap, span_out, n_req) ? DAGPU_OK : DAGPU_ERR_ARG;
}

// ---- namespace search and proofs from a resident square (nmt_namespace.hip) ----

size_t dagpu_nmt_namespace_workspace_size(uint32_t k, size_t n_q) {
  if (k == 0 || !is_pow2(k) || k > (uint32_t)kMaxK) return 0;
  const size_t w = 2 * (size_t)k, pairs = n_q * w;
  // padded queries | ranges of every (query, row) | then, for the proof call:
  // packed requests, node and leaf offsets and absence records of <= pairs proofs
  return ws_align256(32 * n_q) + ws_align256(pairs * kNsRangeWords * sizeof(int32_t)) +
         ws_align256((4 * pairs + 2) * sizeof(int64_t)) + 256;
}

int dagpu_nmt_namespace_ranges_device(dagpu_ctx* ctx, uint32_t k, size_t n_q, const uint8_t* namespaces,
                                      const uint8_t* d_row_nodes, int32_t* ranges_out, int64_t* counts_out,
                                      void* d_workspace, void* stream) {
  int rc = check_ctx_k(ctx, k);
  if (rc) return rc;
  if (n_q == 0) return ns_zero_counts(counts_out);
  if (!ranges_out || !counts_out) return set_err(ctx, DAGPU_ERR_ARG, "dagpu_nmt_namespace_ranges_device: null buffer");
  rc = ns_common_check(ctx, "dagpu_nmt_namespace_ranges_device", namespaces, d_row_nodes, d_workspace);
  if (rc) return rc;
  return ns_search(ctx, k, n_q, namespaces, d_row_nodes, ranges_out, counts_out, (uint8_t*)d_workspace,
                   (hipStream_t)stream);
}

int dagpu_nmt_prove_namespace_batch_device(dagpu_ctx* ctx, uint32_t k, size_t n_q, const uint8_t* namespaces,
                                           const uint8_t* d_eds, const uint8_t* d_row_nodes, uint8_t* d_nodes_out,
                                           size_t nodes_cap, uint8_t* d_ns_out, uint8_t* d_shares_out,
                                           size_t shares_cap, uint8_t* d_leaf_hashes_out, size_t leaf_hashes_cap,
                                           int64_t* desc_out, int32_t* pairs_out, size_t proofs_cap,
                                           int64_t* counts_out, void* d_workspace, void* stream) {
  int rc = check_ctx_k(ctx, k);
  if (rc) return rc;
  if (n_q == 0) return ns_zero_counts(counts_out);
  const std::string who = "dagpu_nmt_prove_namespace_batch_device";
  if (!counts_out || !d_ns_out || !d_eds || (nodes_cap && !d_nodes_out) || (shares_cap && !d_shares_out) ||
      (leaf_hashes_cap && !d_leaf_hashes_out) || (proofs_cap && (!desc_out || !pairs_out)))
    return set_err(ctx, DAGPU_ERR_ARG, who + ": null buffer");
  rc = ns_common_check(ctx, who, namespaces, d_row_nodes, d_workspace);
  if (rc) return rc;
  if ((((uintptr_t)d_eds | (uintptr_t)d_shares_out) & 15) != 0 ||
      ((((uintptr_t)d_nodes_out) | (uintptr_t)d_leaf_hashes_out) & 1) != 0)
    return set_err(ctx, DAGPU_ERR_ARG, who + ": misaligned buffer");
  hipStream_t s = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)d_workspace;
  const size_t w = 2 * (size_t)k, pairs = n_q * w;
  const int m = prove_log2((uint32_t)w);
  std::vector<int32_t> ranges(pairs * kNsRangeWords);
  int64_t need[4];
  rc = ns_search(ctx, k, n_q, namespaces, d_row_nodes, ranges.data(), need, ws, s);
  if (rc) return rc;
  memcpy(counts_out, need, sizeof need);
  rc = ns_check_capacity(ctx, who, need, proofs_cap, leaf_hashes_cap, nodes_cap, shares_cap);
  if (rc) return rc;
  const size_t n = (size_t)need[0], n_abs = (size_t)need[1];
  if (n) {
    // device image: packed requests (n) | node_off (n + 1) | leaf_off (n + 1) | absence records (n_abs)
    std::vector<int64_t> meta(3 * n + 2 + n_abs);
    int64_t* node_off = meta.data() + n;
    int64_t* leaf_off = node_off + (n + 1);
    int64_t* abs_rec = leaf_off + (n + 1);
    int64_t nodes = 0, cells = 0;
    size_t i = 0, j = 0;
    for (size_t p = 0; p < pairs; p++) {
      const int32_t* r = ranges.data() + p * kNsRangeWords;
      if (r[0] == kNsOutside) continue;
      const int64_t q = (int64_t)(p / w), row = (int64_t)(p % w);
      const int64_t req[kProveReqWords] = {0, row, r[1], r[2]};
      const int64_t nn = prove_node_count(m, (uint32_t)r[1], (uint32_t)r[2]);
      const bool absent = r[0] == kNsAbsent;
      meta[i] = (int64_t)prove_pack_req(req);
      node_off[i] = nodes;
      leaf_off[i] = cells;
      int64_t* d = desc_out + i * kPvDescNmtNs;
      d[0] = r[1];
      d[1] = r[2];
      d[2] = absent ? 0 : r[2] - r[1];
      d[3] = cells;
      d[4] = nn;
      d[5] = nodes;
      d[6] = q;
      d[7] = row;
      d[8] = absent ? (int64_t)j : -1;
      pairs_out[2 * i] = (int32_t)q;
      pairs_out[2 * i + 1] = (int32_t)row;
      if (absent) abs_rec[j++] = row * (int64_t)w + r[1];
      nodes += nn;
      if (!absent) cells += r[2] - r[1];
      i++;
    }
    node_off[n] = nodes;
    leaf_off[n] = cells;
    uint8_t* d_meta = ws + ws_align256(32 * n_q) + ws_align256(pairs * kNsRangeWords * sizeof(int32_t));
    HIP_TRY(ctx, hipMemcpyAsync(d_meta, meta.data(), meta.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));  // `meta` may go
    ProveArgs a = prove_args(k, d_row_nodes, nullptr, nullptr, ProofStoreLayout{}, d_eds, 0);
    prove_tables(&a, 1, n, (const int64_t*)d_meta, (const int64_t*)d_meta + n, (const int64_t*)d_meta + 2 * n + 1, nodes,
                 cells);
    a.nodes_out = d_nodes_out;
    a.shares_out = d_shares_out;
    rc = prove_launch(ctx, a, s);
    if (rc) return rc;
    HIP_TRY(ctx, launch_ns_leaf_nodes(d_row_nodes, (const int64_t*)d_meta + 3 * n + 2, (long)n_abs, d_leaf_hashes_out, s));
  }
  // the query namespaces, as uploaded for the search (zero padded to 32 B each)
  HIP_TRY(ctx, hipMemcpy2DAsync(d_ns_out, kNsSize, ws, 32, kNsSize, n_q, hipMemcpyDeviceToDevice, s));
  return DAGPU_OK;
}

// ---- the same across the squares of a batch proof store (ns_squares_layout.hpp) ----

size_t dagpu_nmt_namespace_squares_workspace_size(uint32_t k, size_t n_sq, size_t n_q, size_t proofs_cap) {
  NsSqCarve c;
  if (k == 0 || !is_pow2(k) || k > (uint32_t)kMaxK || !ns_squares_carve(k, n_sq, n_q, proofs_cap, &c)) return 0;
  return c.total;
}

int dagpu_nmt_namespace_squares_count_device(dagpu_ctx* ctx, uint32_t k, size_t n_sq, size_t n_q,
                                             const uint8_t* namespaces, const uint8_t* d_store, int64_t* counts_out,
                                             int32_t* per_out, void* d_workspace, void* stream) {
  int rc = check_ctx_k(ctx, k);
  if (rc) return rc;
  const std::string who = "dagpu_nmt_namespace_squares_count_device";
  if (n_sq == 0) return set_err(ctx, DAGPU_ERR_ARG, who + ": no squares");
  if (n_q == 0) return ns_zero_counts(counts_out);
  if (!counts_out) return set_err(ctx, DAGPU_ERR_ARG, who + ": null buffer");
  NsSqCarve c;
  ProofStoreLayout l;
  rc = ns_sq_common_check(ctx, who, k, n_sq, n_q, 0, namespaces, d_store, d_workspace, &c, &l);
  if (rc) return rc;
  NsSqArgs a;
  return ns_sq_search(ctx, k, n_sq, n_q, namespaces, d_store, c, l.row_bytes, counts_out, per_out,
                      (uint8_t*)d_workspace, (hipStream_t)stream, &a);
}

int dagpu_nmt_prove_namespace_squares_device(dagpu_ctx* ctx, uint32_t k, size_t n_sq, size_t n_q,
                                             const uint8_t* namespaces, const uint8_t* d_eds, size_t square_stride,
                                             const uint8_t* d_store, uint8_t* d_nodes_out, size_t nodes_cap,
                                             uint8_t* d_ns_out, uint8_t* d_shares_out, size_t shares_cap,
                                             uint8_t* d_leaf_hashes_out, size_t leaf_hashes_cap,
                                             uint8_t* d_axis_roots_out, uint8_t* d_dah_leaf_hash_out,
                                             uint8_t* d_aunts_out, int64_t* desc_out, int64_t* mdesc_out,
                                             int32_t* hits_out, size_t proofs_cap, int64_t* counts_out,
                                             void* d_workspace, void* stream) {
  int rc = check_ctx_k(ctx, k);
  if (rc) return rc;
  const std::string who = "dagpu_nmt_prove_namespace_squares_device";
  if (n_sq == 0) return set_err(ctx, DAGPU_ERR_ARG, who + ": no squares");
  if (n_q == 0) return ns_zero_counts(counts_out);
  if (!counts_out || !d_ns_out || !d_eds || (nodes_cap && !d_nodes_out) || (shares_cap && !d_shares_out) ||
      (leaf_hashes_cap && !d_leaf_hashes_out) || (proofs_cap && (!desc_out || !hits_out)))
    return set_err(ctx, DAGPU_ERR_ARG, who + ": null buffer");
  NsSqCarve c;
  ProofStoreLayout l;
  rc = ns_sq_common_check(ctx, who, k, n_sq, n_q, proofs_cap, namespaces, d_store, d_workspace, &c, &l);
  if (rc) return rc;
  if ((((uintptr_t)d_eds | (uintptr_t)d_shares_out | (uintptr_t)d_dah_leaf_hash_out | (uintptr_t)d_aunts_out |
        square_stride) & 15) != 0 ||
      ((((uintptr_t)d_nodes_out) | (uintptr_t)d_leaf_hashes_out | (uintptr_t)d_axis_roots_out) & 1) != 0)
    return set_err(ctx, DAGPU_ERR_ARG, who + ": misaligned buffer");
  const size_t w = 2 * (size_t)k;
  if (square_stride < w * w * kShareSize)
    return set_err(ctx, DAGPU_ERR_ARG, who + ": square_stride smaller than a square");
  hipStream_t s = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)d_workspace;
  NsSqArgs f;
  int64_t need[kNsSqSums];
  rc = ns_sq_search(ctx, k, n_sq, n_q, namespaces, d_store, c, l.row_bytes, need, nullptr, ws, s, &f);
  if (rc) return rc;
  memcpy(counts_out, need, sizeof need);
  rc = ns_check_capacity(ctx, who, need, proofs_cap, leaf_hashes_cap, nodes_cap, shares_cap);
  if (rc) return rc;
  const size_t n = (size_t)need[0];
  if (n) {
    // the tables of the emit kernels are written on the device; only the hit
    // records come back, and they are re-checked before anything is emitted
    std::vector<uint32_t> rec(n * kNsHitRecWords);
    std::vector<int32_t> hits(n * kNsHitWords);
    HIP_TRY(ctx, launch_ns_sq_scatter(f, s));
    HIP_TRY(ctx, hipMemcpyAsync(rec.data(), f.hits, rec.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (!ns_sq_check_hits(n, rec.data(), n_q, n_sq, (uint32_t)w, need, hits.data()))
      return set_err(ctx, DAGPU_ERR_DEVICE, "namespace search returned a hit outside the batch");
    ProveArgs a = prove_args(k, d_store, d_store + l.col_off, d_store + l.dah_off, l, d_eds, square_stride);
    prove_tables(&a, 2, n, f.req, f.node_off, f.leaf_off, need[2], need[3]);
    a.nodes_out = d_nodes_out;
    a.shares_out = d_shares_out;
    a.axis_roots_out = d_axis_roots_out;
    a.leaf_hash_out = d_dah_leaf_hash_out;
    a.aunts_out = d_aunts_out;
    HIP_TRY(ctx, launch_prove_emit(a, s));
    HIP_TRY(ctx, launch_prove_shares(a, s));
    HIP_TRY(ctx, launch_ns_leaf_nodes(d_store, f.abs_rec, (long)need[1], d_leaf_hashes_out, s));
    if (d_axis_roots_out || d_dah_leaf_hash_out || d_aunts_out) HIP_TRY(ctx, launch_prove_sq_merkle(a, s));
    memcpy(hits_out, hits.data(), hits.size() * sizeof(int32_t));
    ns_sq_fill_desc(k, n, hits.data(), desc_out, mdesc_out);
  }
  // the query namespaces, as uploaded for the search (zero padded to 32 B each)
  HIP_TRY(ctx, hipMemcpy2DAsync(d_ns_out, kNsSize, ws + c.queries, 32, kNsSize, n_q, hipMemcpyDeviceToDevice, s));
  return DAGPU_OK;
}

}  // extern "C"
