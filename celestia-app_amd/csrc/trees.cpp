// trees.cpp -- C ABI for batched generic trees on the GPU (include/dagpu.h):
//   dagpu_nmt_roots        nmt.New(sha256, NamespaceIDSize(29), IgnoreMaxNamespace)
//                          Push*/Root (nmt v0.20.0; hasher mirror
//                          test/util/malicious/hasher.go:161-309)
//   dagpu_wrapper_roots    wrapper.ErasuredNamespacedMerkleTree Push/Root as the
//                          rsmt2d.Tree of wrapper.NewConstructor
//                          (pkg/wrapper/nmt_wrapper.go:55-124)
//   dagpu_merkle_roots     merkle.HashFromByteSlices (celestia-core crypto/merkle)
//   dagpu_blob_commitments inclusion.CreateCommitment over already-split blob
//                          shares (pkg/inclusion/commitment.go:19-75,
//                          blob_share_commitment_rules.go:76-101)
//   dagpu_nmt_verify_batch / dagpu_nmt_verify_batch_device / dagpu_merkle_verify_batch
//                          nmt Proof.VerifyInclusion and crypto/merkle Proof.Verify
//                          for many proofs (celestia-core ShareProof.Validate /
//                          RowProof.Validate; consumer x/blobstream/client/verify.go:216-227),
//                          hashed on the device (proof_verify.hip)
//   dagpu_row_nodes_device / dagpu_col_nodes_device
//                          every node of the row and column trees of a resident
//                          square, the stores the proof producer selects from
//                          (prove_host.cpp, nmt_prove.hip)
//   dagpu_nmt_verify_namespace / dagpu_nmt_verify_namespace_batch(_device)
//                          nmt Proof.VerifyNamespace: presence with completeness,
//                          absence and empty proofs (rules stated in dagpu.h,
//                          recalled from nmt v0.20.0); the fold is shared with
//                          VerifyInclusion (nmt_fold_verify)
// Each call uploads the pushes once, hashes every leaf and level of every
// tree in a handful of launches (nmt_forest.hip) and returns the roots.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <string>
#include <functional>
#include <vector>

#include "../../include/dagpu.h"
#include "forest.hpp"
#include "kernels.hpp"
#include "host_sha256.hpp"
#include "pipe_carve.hpp"
#include "proof_verify.hpp"
#include "runtime.hpp"

namespace {

long round4(long v) { return (v + 3) & ~3L; }

// Upload `n` leaves of `len` bytes (packed on the host) into a 4-B aligned
// device array with stride round4(len).
int upload_leaves(dagpu_ctx* ctx, const uint8_t* host, long n, long len, long* stride_out,
                  hipStream_t s) {
  const long stride = round4(len < 1 ? 1 : len);
  *stride_out = stride;
  HIP_TRY(ctx, ctx->t_leaf_data.ensure((size_t)(stride * (n > 0 ? n : 1))));
  if (n == 0 || len == 0) return DAGPU_OK;
  if (stride == len) {
    HIP_TRY(ctx, hipMemcpyAsync(ctx->t_leaf_data.p, host, (size_t)(n * len), hipMemcpyHostToDevice, s));
  } else {
    HIP_TRY(ctx, hipMemcpy2DAsync(ctx->t_leaf_data.p, (size_t)stride, host, (size_t)len, (size_t)len,
                                  (size_t)n, hipMemcpyHostToDevice, s));
  }
  return DAGPU_OK;
}

// One NMT forest over leaves already in ctx->t_leaf_data; roots to host.
int nmt_forest_host(dagpu_ctx* ctx, const std::vector<long>& counts, long dlen, long stride, int pmode,
                    const uint8_t* flags_host, int ignore_max, uint8_t* roots, int32_t* status,
                    hipStream_t s) {
  const long T = (long)counts.size();
  long nleaves = 0;
  for (long c : counts) nleaves += c;
  ForestPlan plan = ForestPlan::ragged_plan(counts);
  HIP_TRY(ctx, ctx->t_leaves.ensure((size_t)(kRecNmt * (nleaves > 0 ? nleaves : 1))));
  HIP_TRY(ctx, ctx->t_inner.ensure((size_t)(kRecNmt * (plan.inner_records > 0 ? plan.inner_records : 1))));
  HIP_TRY(ctx, ctx->t_meta.ensure(plan.meta.size() * sizeof(int64_t) + 8));
  HIP_TRY(ctx, ctx->t_out.ensure((size_t)(kNodeSize * T + 16)));
  HIP_TRY(ctx, ctx->t_status.ensure((size_t)(4 * T + 4)));
  HIP_TRY(ctx, hipMemsetAsync(ctx->t_status.p, 0, (size_t)(4 * T + 4), s));
  if (pmode == kPfxFlags) {
    HIP_TRY(ctx, ctx->t_flags.ensure((size_t)(nleaves + 1)));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->t_flags.p, flags_host, (size_t)nleaves, hipMemcpyHostToDevice, s));
  }
  ForestLeafArgs la{};
  la.data = (const uint8_t*)ctx->t_leaf_data.p;
  la.data_stride = stride;
  la.dlen = dlen;
  la.nleaves = nleaves;
  la.pmode = pmode;
  la.pflags = (const uint8_t*)ctx->t_flags.p;
  la.rfc = 0;
  la.out = (uint8_t*)ctx->t_leaves.p;
  HIP_TRY(ctx, launch_forest_leaves(la, s));
  HIP_TRY(ctx, forest_enqueue(plan, (const uint8_t*)ctx->t_leaves.p, (uint8_t*)ctx->t_inner.p,
                              (int64_t*)ctx->t_meta.p, ignore_max, 1, 0, (int32_t*)ctx->t_status.p,
                              (uint8_t*)ctx->t_out.p, 0, 0, s));
  std::vector<int32_t> st(T);
  if (T) {
    HIP_TRY(ctx, hipMemcpyAsync(roots, ctx->t_out.p, (size_t)(kNodeSize * T), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(st.data(), ctx->t_status.p, (size_t)(4 * T), hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(ctx, hipStreamSynchronize(s));  // also keeps `plan` alive past its upload
  int first = DAGPU_OK;
  for (long t = 0; t < T; t++) {
    const int v = (st[t] & kForestPushOrder) ? DAGPU_ERR_PUSH_ORDER : DAGPU_OK;
    if (status) status[t] = v;
    if (v && !first) first = v;
  }
  if (first) set_err(ctx, first, "invalid push order: pushed namespace is smaller than the last one");
  return first;
}

// RoundUpPowerOfTwo (pkg/shares/powers_of_two.go:10-16)
uint64_t round_up_pow2(uint64_t v) {
  uint64_t r = 1;
  while (r < v) r <<= 1;
  return r;
}

// inclusion.SubTreeWidth (pkg/inclusion/blob_share_commitment_rules.go:85-101)
uint64_t subtree_width(uint64_t share_count, uint64_t threshold) {
  uint64_t s = share_count / threshold;
  if (share_count % threshold != 0) s++;
  s = round_up_pow2(s);
  const uint64_t min_sq = round_up_pow2((uint64_t)std::ceil(std::sqrt((double)share_count)));
  return s < min_sq ? s : min_sq;
}

// inclusion.MerkleMountainRangeSizes (pkg/inclusion/commitment.go:85-107)
std::vector<long> mmr_sizes(uint64_t total, uint64_t max_tree) {
  std::vector<long> out;
  while (total != 0) {
    if (total >= max_tree) {
      out.push_back((long)max_tree);
      total -= max_tree;
    } else {
      const uint64_t up = round_up_pow2(total);
      const uint64_t t = up == total ? up : up / 2;
      out.push_back((long)t);
      total -= t;
    }
  }
  return out;
}

// The fold of nmt Proof.VerifyInclusion and Proof.VerifyNamespace over n leaf
// nodes (90 B each) proven at [start, end), start < end.  With `nid` the
// completeness rule of VerifyNamespace holds too: a proof node consumed left of
// the range must have max < nid, one consumed right of it (the leftover nodes
// folded on the right included) nid < min.
int nmt_fold_verify(const uint8_t* lh, size_t n, int64_t start, int64_t end, const uint8_t* nodes, size_t nnodes,
                    const uint8_t* root90, const uint8_t* nid) {
  using namespace dagpu::host;
  size_t next_leaf = 0, next_node = 0;
  bool ok = true;
  auto complete = [&](const uint8_t* node, bool left) {
    if (!nid) return;
    if (left ? !(memcmp(node + kNs, nid, kNs) < 0) : !(memcmp(nid, node, kNs) < 0)) ok = false;
  };
  // nmt getSplitPoint: largest power of two strictly below length (length >= 2)
  auto split = [](int64_t len) {
    int64_t k = 1;
    while (k * 2 < len) k *= 2;
    return k;
  };
  // verifyLeafHashes.computeRoot: proof nodes fill the subtrees disjoint from
  // [start, end), popped left to right; an absent right subtree is skipped.
  std::function<bool(int64_t, int64_t, uint8_t*)> root_of = [&](int64_t lo, int64_t hi, uint8_t* out) -> bool {
    if (hi - lo == 1 && start <= lo && lo < end) {
      memcpy(out, &lh[next_leaf++ * kNodeLen], kNodeLen);
      return true;
    }
    if (hi - lo == 1 || hi <= start || lo >= end) {
      if (next_node >= nnodes) return false;
      complete(nodes + next_node * kNodeLen, hi <= start);
      memcpy(out, nodes + next_node++ * kNodeLen, kNodeLen);
      return true;
    }
    const int64_t k = split(hi - lo);
    uint8_t l[kNodeLen], r[kNodeLen];
    if (!root_of(lo, lo + k, l)) return false;  // a missing left subtree cannot verify
    if (!root_of(lo + k, hi, r)) {
      memcpy(out, l, kNodeLen);
      return true;
    }
    if (!nmt_hash_node(l, r, out)) ok = false;
    return true;
  };
  int64_t est = 1;
  while (est < end) est *= 2;  // getSplitPoint(end) * 2: the subtree holding the range
  uint8_t root[kNodeLen];
  if (!root_of(0, est, root)) return DAGPU_ERR_PROOF;
  for (; next_node < nnodes; next_node++) {  // remaining right-hand nodes
    uint8_t t[kNodeLen];
    complete(nodes + next_node * kNodeLen, false);
    if (!nmt_hash_node(root, nodes + next_node * kNodeLen, t)) ok = false;
    memcpy(root, t, kNodeLen);
  }
  if (!ok || next_leaf != n) return DAGPU_ERR_PROOF;
  return memcmp(root, root90, kNodeLen) == 0 ? DAGPU_OK : DAGPU_ERR_PROOF;
}

// ---- batched proof verification (proof_verify.hip) ----

// off >= 0, cnt >= 0 and [off, off + cnt) inside [0, total)
bool pv_span_ok(int64_t off, int64_t cnt, size_t total) {
  return off >= 0 && cnt >= 0 && (uint64_t)off <= (uint64_t)total && (uint64_t)cnt <= (uint64_t)total - (uint64_t)off;
}

// A range nmt Proof.VerifyInclusion rejects before it hashes (trees.cpp
// dagpu_nmt_verify_inclusion).  end > 2^62: the host verifier's doubling of
// `est` cannot reach it; no tree is that wide.
bool pv_range_rejected(const int64_t* d) {
  const int64_t start = d[0], end = d[1], nl = d[2];
  return start < 0 || start >= end || end > ((int64_t)1 << kPvMaxHeight) || nl != end - start;
}

// Leaf records of a 9-word namespace descriptor (dagpu_nmt_verify_namespace):
// 0 when the host verifier rejects it before it hashes, and for the empty form,
// which the fold kernel decides against the root; 1 for an absence proof (its
// leaf hash; nid < leafHash.min is tested on the device, where the tables
// are); n_leaves for a presence proof.
int64_t pv_ns_records(const int64_t* d) {
  const int64_t start = d[0], end = d[1], nl = d[2], nn = d[4], lh = d[8];
  if (start == end && nn == 0 && lh < 0) return 0;
  if (start < 0 || start >= end || end > ((int64_t)1 << kPvMaxHeight)) return 0;
  if (lh >= 0) return nl == 0 && end - start == 1 ? 1 : 0;
  return nl == end - start ? nl : 0;
}

// Host image of what the nmt kernels read besides the bulk data.
struct PvNmtPlan {
  std::vector<int64_t> meta;  // desc (8 n, or 9 n) | rec_off (n + 1) | cs_off (n + 1)
  long n_records = 0, n_stack = 0;
};

// Every descriptor against the totals; nothing is launched when one fails.
// words = kPvDescNmt, or kPvDescNmtNs with the leaf-hash table of n_lh entries.
int pv_check_nmt(dagpu_ctx* ctx, size_t n, const int64_t* desc, size_t n_ns, size_t n_leaves, size_t n_nodes,
                 size_t n_roots, PvNmtPlan* plan, int words = kPvDescNmt, size_t n_lh = 0) {
  const bool ns_rules = words == kPvDescNmtNs;
  plan->meta.resize(n * words + 2 * (n + 1));
  int64_t* rec_off = plan->meta.data() + n * words;
  int64_t* cs_off = rec_off + (n + 1);
  long recs = 0, stack = 0;
  for (size_t i = 0; i < n; i++) {
    const int64_t* d = desc + i * words;
    if (!pv_span_ok(d[3], d[2], n_leaves) || !pv_span_ok(d[5], d[4], n_nodes) || d[4] > INT32_MAX ||
        d[6] < 0 || (uint64_t)d[6] >= n_ns || d[7] < 0 || (uint64_t)d[7] >= n_roots ||
        (ns_rules && (d[8] < -1 || (d[8] >= 0 && (uint64_t)d[8] >= n_lh))))
      return set_err(ctx, DAGPU_ERR_ARG, "proof descriptor " + std::to_string(i) + " points outside the buffers");
    memcpy(plan->meta.data() + i * words, d, words * sizeof(int64_t));
    rec_off[i] = recs;
    cs_off[i] = stack;
    const int64_t nrec = ns_rules ? pv_ns_records(d) : pv_range_rejected(d) ? 0 : d[2];
    if (nrec > 0) {
      recs += (long)nrec;
      stack += pv_stack_depth(nrec);
    }
  }
  rec_off[n] = recs;
  cs_off[n] = stack;
  plan->n_records = recs;
  plan->n_stack = stack;
  return DAGPU_OK;
}

size_t pv_nmt_meta_bytes(size_t n, int words = kPvDescNmt) {
  return ws_align256((n * words + 2 * (n + 1)) * sizeof(int64_t));
}

// Upload the plan and enqueue the leaf and fold passes.  Returns once the
// upload is complete (the plan and the caller's descriptors may go).
int pv_nmt_enqueue(dagpu_ctx* ctx, size_t n, const PvNmtPlan& plan, const uint8_t* d_ns, const uint8_t* d_leaves,
                   size_t leaf_len, const uint8_t* d_nodes, const uint8_t* d_roots, int32_t* d_status,
                   uint8_t* d_ws, hipStream_t s, int words = kPvDescNmt, const uint8_t* d_leaf_hashes = nullptr) {
  HIP_TRY(ctx, hipMemcpyAsync(d_ws, plan.meta.data(), plan.meta.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  PvNmtArgs a{};
  a.n = (long)n;
  a.namespace_rules = words == kPvDescNmtNs;
  a.desc = (const int64_t*)d_ws;
  a.rec_off = a.desc + n * words;
  a.cs_off = a.rec_off + (n + 1);
  a.ns = d_ns;
  a.leaves = d_leaves;
  a.leaf_len = (long)leaf_len;
  a.fast512 = leaf_len == (size_t)kShareSize && (((uintptr_t)d_leaves) & 15) == 0;
  a.nodes = d_nodes;
  a.roots = d_roots;
  a.leaf_hashes = d_leaf_hashes;
  a.recs = d_ws + pv_nmt_meta_bytes(n, words);
  a.cstack = a.recs + (size_t)plan.n_records * kRecNmt;
  a.status = d_status;
  HIP_TRY(ctx, launch_pv_nmt_leaves(a, plan.n_records, s));
  HIP_TRY(ctx, launch_pv_nmt_fold(a, s));
  return DAGPU_OK;
}

// One device allocation for a host-form call, freed on every path.
struct PvScratch {
  void* p = nullptr;
  ~PvScratch() {
    if (p) (void)hipFree(p);
  }
};

}  // namespace

extern "C" {

int dagpu_nmt_roots(dagpu_ctx* ctx, size_t ntrees, const uint32_t* leaf_counts, const uint8_t* leaves,
                    size_t leaf_len, int prefix_mode, const uint8_t* prefix_flags, int ignore_max_ns,
                    uint8_t* roots, int32_t* status) {
  if (!ctx || (ntrees && (!leaf_counts || !roots))) return DAGPU_ERR_ARG;
  if (prefix_mode < DAGPU_PREFIX_NONE || prefix_mode > DAGPU_PREFIX_FLAGS) return DAGPU_ERR_ARG;
  std::lock_guard<std::mutex> g(ctx->mu);
  (void)hipSetDevice(ctx->device);
  std::vector<long> counts(ntrees);
  long n = 0;
  for (size_t t = 0; t < ntrees; t++) n += (counts[t] = leaf_counts[t]);
  if (n && !leaves) return DAGPU_ERR_ARG;
  if (prefix_mode == DAGPU_PREFIX_FLAGS && n && !prefix_flags) return DAGPU_ERR_ARG;
  // nmt HashLeaf / Push: namespaced data shorter than the namespace is rejected
  // (ErrInvalidLeafLen / ErrMismatchedNamespaceSize); prepending modes need the
  // namespace inside the data only for DAGPU_PREFIX_SELF.
  const bool need_ns = prefix_mode == DAGPU_PREFIX_NONE || prefix_mode == DAGPU_PREFIX_SELF ||
                       prefix_mode == DAGPU_PREFIX_FLAGS;
  if (n && need_ns && leaf_len < (size_t)kNsSize)
    return set_err(ctx, DAGPU_ERR_SHARE_SIZE, "invalid leaf length: shorter than the namespace size");
  if (prefix_mode == DAGPU_PREFIX_FLAGS)
    for (long i = 0; i < n; i++)
      if (prefix_flags[i] != DAGPU_PREFIX_SELF && prefix_flags[i] != DAGPU_PREFIX_PARITY) return DAGPU_ERR_ARG;
  hipStream_t s = ctx->stream;
  long stride = 0;
  int rc = upload_leaves(ctx, leaves, n, (long)leaf_len, &stride, s);
  if (rc) return rc;
  return nmt_forest_host(ctx, counts, (long)leaf_len, stride, prefix_mode, prefix_flags, ignore_max_ns != 0,
                         roots, status, s);
}

int dagpu_wrapper_roots(dagpu_ctx* ctx, uint64_t square_size, size_t ntrees, const uint32_t* axis_index,
                        const uint32_t* leaf_counts, const uint8_t* shares, size_t share_len,
                        uint8_t* roots, int32_t* status) {
  if (!ctx || (ntrees && (!axis_index || !leaf_counts || !roots))) return DAGPU_ERR_ARG;
  // NewErasuredNamespacedMerkleTree panics on squareSize == 0 (nmt_wrapper.go:56-58)
  if (square_size == 0) return set_err(ctx, DAGPU_ERR_ARG, "cannot create a ErasuredNamespacedMerkleTree of squareSize == 0");
  long n = 0;
  for (size_t t = 0; t < ntrees; t++) {
    // Push bounds check (nmt_wrapper.go:94-96)
    if ((uint64_t)axis_index[t] + 1 > 2 * square_size || (uint64_t)leaf_counts[t] > 2 * square_size) {
      if (status) status[t] = DAGPU_ERR_ARG;
      char buf[160];
      snprintf(buf, sizeof buf, "pushed past predetermined square size: boundary at %llu index at %u %u",
               (unsigned long long)(2 * square_size), axis_index[t],
               leaf_counts[t] ? leaf_counts[t] - 1 : 0);
      return set_err(ctx, DAGPU_ERR_ARG, buf);
    }
    n += leaf_counts[t];
  }
  if (n && !shares) return DAGPU_ERR_ARG;
  // nmt_wrapper.go:97-99
  if (n && share_len < (size_t)kNsSize)
    return set_err(ctx, DAGPU_ERR_SHARE_SIZE, "data is too short to contain namespace ID");
  // isQuadrantZero (nmt_wrapper.go:138-140): shareIndex < k && axisIndex < k
  std::vector<uint8_t> flags((size_t)n);
  long i = 0;
  for (size_t t = 0; t < ntrees; t++)
    for (uint32_t j = 0; j < leaf_counts[t]; j++, i++)
      flags[i] = (j < square_size && axis_index[t] < square_size) ? DAGPU_PREFIX_SELF : DAGPU_PREFIX_PARITY;
  return dagpu_nmt_roots(ctx, ntrees, leaf_counts, shares, share_len, DAGPU_PREFIX_FLAGS, flags.data(), 1,
                         roots, status);
}

int dagpu_merkle_roots(dagpu_ctx* ctx, size_t ntrees, const uint32_t* counts, const uint8_t* items,
                       size_t item_len, uint8_t* out32) {
  if (!ctx || (ntrees && (!counts || !out32))) return DAGPU_ERR_ARG;
  std::lock_guard<std::mutex> g(ctx->mu);
  (void)hipSetDevice(ctx->device);
  std::vector<long> cnt(ntrees);
  long n = 0;
  for (size_t t = 0; t < ntrees; t++) n += (cnt[t] = counts[t]);
  if (n && !items) return DAGPU_ERR_ARG;
  hipStream_t s = ctx->stream;
  long stride = 0;
  int rc = upload_leaves(ctx, items, n, (long)item_len, &stride, s);
  if (rc) return rc;
  ForestPlan plan = ForestPlan::ragged_plan(cnt);
  HIP_TRY(ctx, ctx->t_leaves.ensure((size_t)(kRecRfc * (n > 0 ? n : 1))));
  HIP_TRY(ctx, ctx->t_inner.ensure((size_t)(kRecRfc * (plan.inner_records > 0 ? plan.inner_records : 1))));
  HIP_TRY(ctx, ctx->t_meta.ensure(plan.meta.size() * sizeof(int64_t) + 8));
  HIP_TRY(ctx, ctx->t_out.ensure((size_t)(32 * ntrees + 16)));
  ForestLeafArgs la{};
  la.data = (const uint8_t*)ctx->t_leaf_data.p;
  la.data_stride = stride;
  la.dlen = (long)item_len;
  la.nleaves = n;
  la.pmode = kPfxNone;
  la.rfc = 1;
  la.out = (uint8_t*)ctx->t_leaves.p;
  HIP_TRY(ctx, launch_forest_leaves(la, s));
  HIP_TRY(ctx, forest_enqueue(plan, (const uint8_t*)ctx->t_leaves.p, (uint8_t*)ctx->t_inner.p,
                              (int64_t*)ctx->t_meta.p, 0, 0, 1, nullptr, (uint8_t*)ctx->t_out.p, 0, 0, s));
  if (ntrees) HIP_TRY(ctx, hipMemcpyAsync(out32, ctx->t_out.p, 32 * ntrees, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  return DAGPU_OK;
}

size_t dagpu_row_nodes_size(uint32_t k) {
  if (k == 0 || !is_pow2(k) || k > (uint32_t)kMaxK) return 0;
  const long w = 2L * k;
  long recs = 0;
  for (long per = w; per >= 1; per >>= 1) recs += w * per;
  return (size_t)recs * kRecNmt;
}

size_t dagpu_row_nodes_workspace_size(uint32_t k) {
  if (k == 0 || !is_pow2(k) || k > (uint32_t)kMaxK) return 0;
  const long w = 2L * k;
  return (size_t)w * sizeof(int64_t) + 256;  // plan metadata (root indices)
}

int dagpu_row_nodes_device(dagpu_ctx* ctx, uint32_t k, const uint8_t* d_eds, uint8_t* d_nodes, void* d_workspace,
                           void* stream) {
  if (!ctx || !d_eds || !d_nodes || !d_workspace) return DAGPU_ERR_ARG;
  int rc = check_k(ctx, k);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const long w = 2L * k;
  // leaves (level 0): every cell with the wrapper namespace rule, row-major
  ForestLeafArgs la{};
  la.data = d_eds;
  la.data_stride = kShareSize;
  la.dlen = kShareSize;
  la.nleaves = w * w;
  la.pmode = kPfxGrid;
  la.grid_k = (int)k;
  la.grid_w = w;
  la.out = d_nodes;
  HIP_TRY(ctx, launch_forest_leaves(la, s));
  // every row tree, all levels kept: level L packed right after level L-1
  ForestPlan plan = ForestPlan::uniform_plan(w, w, w, 1);
  HIP_TRY(ctx, forest_enqueue(plan, d_nodes, d_nodes + (size_t)w * w * kRecNmt, (int64_t*)d_workspace, 1, 0, 0,
                              nullptr, d_nodes + (size_t)w * w * kRecNmt + (size_t)plan.base[plan.nlevels] * kRecNmt,
                              1, 0, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));  // plan metadata upload complete
  return DAGPU_OK;
}

int dagpu_row_nodes_gather_device(dagpu_ctx* ctx, uint32_t k, const uint8_t* d_nodes, size_t n,
                                  const uint32_t* d_requests, uint8_t* d_out, void* stream) {
  if (!ctx || !d_nodes || (n && (!d_requests || !d_out))) return DAGPU_ERR_ARG;
  int rc = check_k(ctx, k);
  if (rc) return rc;
  HIP_TRY(ctx, launch_node_gather(d_nodes, 2 * (int)k, d_requests, (long)n, d_out, (hipStream_t)stream));
  return DAGPU_OK;
}

size_t dagpu_col_nodes_size(uint32_t k) {
  const size_t rows = dagpu_row_nodes_size(k);
  return rows ? rows - (size_t)(2L * k) * (size_t)(2L * k) * kRecNmt : 0;
}

size_t dagpu_col_nodes_workspace_size(uint32_t k) {
  if (k == 0 || !is_pow2(k) || k > (uint32_t)kMaxK) return 0;
  return 256;  // the uniform plan addresses its levels by shape: nothing is uploaded
}

int dagpu_col_nodes_device(dagpu_ctx* ctx, uint32_t k, const uint8_t* d_row_nodes, uint8_t* d_col_inner,
                           void* d_workspace, void* stream) {
  if (!ctx || !d_row_nodes || !d_col_inner || !d_workspace) return DAGPU_ERR_ARG;
  int rc = check_k(ctx, k);
  if (rc) return rc;
  if (((uintptr_t)d_row_nodes | (uintptr_t)d_col_inner) & 15)
    return set_err(ctx, DAGPU_ERR_ARG, "dagpu_col_nodes_device: node stores must be 16-B aligned");
  hipStream_t s = (hipStream_t)stream;
  const long w = 2L * k;
  // every column tree over the row store's leaf records (tree c: leaf r at
  // r * w + c), all inner levels kept; the top level is the column roots
  ForestPlan plan = ForestPlan::uniform_plan(w, w, 1, w);
  HIP_TRY(ctx, forest_enqueue(plan, d_row_nodes, d_col_inner, (int64_t*)d_workspace, 1, 0, 0, nullptr,
                              d_col_inner + (size_t)plan.base[plan.nlevels] * kRecNmt, 1, 0, s));
  return DAGPU_OK;
}

int dagpu_merkle_levels(dagpu_ctx* ctx, size_t n, const uint8_t* items, size_t item_len, uint8_t* out32,
                        size_t* n_nodes) {
  if (!ctx || !n_nodes || (n && (!items || !out32))) return DAGPU_ERR_ARG;
  std::lock_guard<std::mutex> g(ctx->mu);
  (void)hipSetDevice(ctx->device);
  std::vector<long> cnt{(long)n};
  ForestPlan plan = ForestPlan::ragged_plan(cnt);
  const size_t total = n + (size_t)plan.inner_records;
  if (*n_nodes < total) {
    *n_nodes = total;
    return set_err(ctx, DAGPU_ERR_ARG, "output too small for every tree level");
  }
  *n_nodes = total;
  if (n == 0) return DAGPU_OK;
  hipStream_t s = ctx->stream;
  long stride = 0;
  int rc = upload_leaves(ctx, items, (long)n, (long)item_len, &stride, s);
  if (rc) return rc;
  HIP_TRY(ctx, ctx->t_leaves.ensure(total * kRecRfc + 64));
  HIP_TRY(ctx, ctx->t_meta.ensure(plan.meta.size() * sizeof(int64_t) + 8));
  HIP_TRY(ctx, ctx->t_out.ensure(64));
  ForestLeafArgs la{};
  la.data = (const uint8_t*)ctx->t_leaf_data.p;
  la.data_stride = stride;
  la.dlen = (long)item_len;
  la.nleaves = (long)n;
  la.pmode = kPfxNone;
  la.rfc = 1;
  la.out = (uint8_t*)ctx->t_leaves.p;
  HIP_TRY(ctx, launch_forest_leaves(la, s));
  uint8_t* inner = (uint8_t*)ctx->t_leaves.p + n * kRecRfc;  // levels right after the leaves
  HIP_TRY(ctx, forest_enqueue(plan, (const uint8_t*)ctx->t_leaves.p, inner, (int64_t*)ctx->t_meta.p, 0, 0, 1,
                              nullptr, (uint8_t*)ctx->t_out.p, 0, 0, s));
  HIP_TRY(ctx, hipMemcpyAsync(out32, ctx->t_leaves.p, total * kRecRfc, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  return DAGPU_OK;
}

int dagpu_nmt_verify_inclusion(const uint8_t* ns29, const uint8_t* leaves, size_t n, size_t leaf_len,
                               int64_t start, int64_t end, const uint8_t* nodes, size_t nnodes,
                               const uint8_t* root90) {
  using namespace dagpu::host;
  if (!ns29 || !root90 || (n && !leaves) || (nnodes && !nodes)) return DAGPU_ERR_ARG;
  // Proof.VerifyInclusion: valid range, one leaf per proven index
  if (start < 0 || start >= end || (int64_t)n != end - start) return DAGPU_ERR_PROOF;
  std::vector<uint8_t> lh(n * kNodeLen);
  for (size_t i = 0; i < n; i++) nmt_hash_leaf(ns29, leaves + i * leaf_len, leaf_len, &lh[i * kNodeLen]);
  return nmt_fold_verify(lh.data(), n, start, end, nodes, nnodes, root90, nullptr);
}

int dagpu_nmt_verify_namespace(const uint8_t* ns29, const uint8_t* leaves, size_t n, size_t leaf_len,
                               int64_t start, int64_t end, const uint8_t* nodes, size_t nnodes,
                               const uint8_t* leaf_hash90, const uint8_t* root90) {
  using namespace dagpu::host;
  if (!ns29 || !root90 || (n && !leaves) || (nnodes && !nodes)) return DAGPU_ERR_ARG;
  // the empty form: nid is outside the root's namespace range and nothing is shipped
  if (start == end && nnodes == 0 && !leaf_hash90) {
    if (n != 0) return DAGPU_ERR_PROOF;
    const bool outside = memcmp(ns29, root90, kNs) < 0 || memcmp(root90 + kNs, ns29, kNs) < 0;
    return outside ? DAGPU_OK : DAGPU_ERR_PROOF;
  }
  if (start < 0 || start >= end || end > ((int64_t)1 << kPvMaxHeight)) return DAGPU_ERR_PROOF;
  if (leaf_hash90) {
    // absence: the leaf node of the first leaf with a larger namespace, no leaf data
    if (n != 0 || end - start != 1 || !(memcmp(ns29, leaf_hash90, kNs) < 0)) return DAGPU_ERR_PROOF;
    return nmt_fold_verify(leaf_hash90, 1, start, end, nodes, nnodes, root90, ns29);
  }
  if ((int64_t)n != end - start) return DAGPU_ERR_PROOF;
  std::vector<uint8_t> lh(n * kNodeLen);
  for (size_t i = 0; i < n; i++) nmt_hash_leaf(ns29, leaves + i * leaf_len, leaf_len, &lh[i * kNodeLen]);
  return nmt_fold_verify(lh.data(), n, start, end, nodes, nnodes, root90, ns29);
}

int dagpu_merkle_verify(const uint8_t* root32, const uint8_t* leaf, size_t leaf_len, int64_t index,
                        int64_t total, const uint8_t* aunts, size_t naunts) {
  using namespace dagpu::host;
  if (!root32 || (leaf_len && !leaf) || (naunts && !aunts)) return DAGPU_ERR_ARG;
  if (total < 0 || index < 0) return DAGPU_ERR_PROOF;
  uint8_t h[32];
  merkle_leaf_hash(leaf, leaf_len, h);
  // crypto/merkle computeHashFromAunts, aunts ordered leaf to root
  std::function<bool(int64_t, int64_t, size_t, uint8_t*)> up = [&](int64_t idx, int64_t tot, size_t na,
                                                                     uint8_t* out) -> bool {
    if (idx >= tot || idx < 0 || tot <= 0) return false;
    if (tot == 1) {
      if (na != 0) return false;
      memcpy(out, h, 32);
      return true;
    }
    if (na == 0) return false;
    int64_t left = 1;
    while (left * 2 < tot) left *= 2;
    uint8_t sub[32];
    const uint8_t* aunt = aunts + (na - 1) * 32;
    if (idx < left) {
      if (!up(idx, left, na - 1, sub)) return false;
      merkle_inner_hash(sub, aunt, out);
    } else {
      if (!up(idx - left, tot - left, na - 1, sub)) return false;
      merkle_inner_hash(aunt, sub, out);
    }
    return true;
  };
  uint8_t root[32];
  if (!up(index, total, naunts, root)) return DAGPU_ERR_PROOF;
  return memcmp(root, root32, 32) == 0 ? DAGPU_OK : DAGPU_ERR_PROOF;
}

size_t dagpu_nmt_verify_workspace_size(size_t n, size_t n_leaves) {
  // descriptors and offsets, one 96-B record per proven leaf, and the fold's
  // record stack: pv_stack_depth(nl) <= nl + 3 per proof
  return pv_nmt_meta_bytes(n) + (size_t)kRecNmt * (2 * n_leaves + 3 * n) + 256;
}

int dagpu_nmt_verify_batch_device(dagpu_ctx* ctx, size_t n, const int64_t* desc, const uint8_t* d_namespaces,
                                  size_t n_ns, const uint8_t* d_leaves, size_t n_leaves, size_t leaf_len,
                                  const uint8_t* d_nodes, size_t n_nodes, const uint8_t* d_roots, size_t n_roots,
                                  int32_t* d_status, void* d_workspace, void* stream) {
  if (!ctx) return DAGPU_ERR_ARG;
  if (n == 0) return DAGPU_OK;
  if (!desc || !d_status || !d_workspace || (((uintptr_t)d_workspace) & 15) != 0 || (n_ns && !d_namespaces) ||
      (n_leaves && leaf_len && !d_leaves) || (n_nodes && !d_nodes) || (n_roots && !d_roots))
    return set_err(ctx, DAGPU_ERR_ARG, "dagpu_nmt_verify_batch_device: null or misaligned buffer");
  PvNmtPlan plan;
  int rc = pv_check_nmt(ctx, n, desc, n_ns, n_leaves, n_nodes, n_roots, &plan);
  if (rc) return rc;
  return pv_nmt_enqueue(ctx, n, plan, d_namespaces, d_leaves, leaf_len, d_nodes, d_roots, d_status,
                        (uint8_t*)d_workspace, (hipStream_t)stream);
}

int dagpu_nmt_verify_batch(dagpu_ctx* ctx, size_t n, const int64_t* desc, const uint8_t* namespaces, size_t n_ns,
                           const uint8_t* leaves, size_t n_leaves, size_t leaf_len, const uint8_t* nodes,
                           size_t n_nodes, const uint8_t* roots, size_t n_roots, int32_t* status) {
  if (!ctx) return DAGPU_ERR_ARG;
  if (n == 0) return DAGPU_OK;
  if (!desc || !status || (n_ns && !namespaces) || (n_leaves && leaf_len && !leaves) || (n_nodes && !nodes) ||
      (n_roots && !roots))
    return set_err(ctx, DAGPU_ERR_ARG, "dagpu_nmt_verify_batch: null buffer");
  PvNmtPlan plan;
  int rc = pv_check_nmt(ctx, n, desc, n_ns, n_leaves, n_nodes, n_roots, &plan);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  (void)hipSetDevice(ctx->device);
  hipStream_t s = ctx->stream;
  const size_t b_ns = n_ns * kNsSize, b_lv = n_leaves * leaf_len, b_nd = n_nodes * kNodeSize,
               b_rt = n_roots * kNodeSize;
  const size_t o_ns = 0, o_lv = o_ns + ws_align256(b_ns), o_nd = o_lv + ws_align256(b_lv), o_rt = o_nd + ws_align256(b_nd),
               o_st = o_rt + ws_align256(b_rt), o_ws = o_st + ws_align256(4 * n);
  const size_t ws = pv_nmt_meta_bytes(n) + (size_t)kRecNmt * (size_t)(plan.n_records + plan.n_stack) + 256;
  PvScratch m;
  HIP_TRY(ctx, hipMalloc(&m.p, o_ws + ws));
  uint8_t* d = (uint8_t*)m.p;
  if (b_ns) HIP_TRY(ctx, hipMemcpyAsync(d + o_ns, namespaces, b_ns, hipMemcpyHostToDevice, s));
  if (b_lv) HIP_TRY(ctx, hipMemcpyAsync(d + o_lv, leaves, b_lv, hipMemcpyHostToDevice, s));
  if (b_nd) HIP_TRY(ctx, hipMemcpyAsync(d + o_nd, nodes, b_nd, hipMemcpyHostToDevice, s));
  if (b_rt) HIP_TRY(ctx, hipMemcpyAsync(d + o_rt, roots, b_rt, hipMemcpyHostToDevice, s));
  rc = pv_nmt_enqueue(ctx, n, plan, d + o_ns, d + o_lv, leaf_len, d + o_nd, d + o_rt, (int32_t*)(d + o_st),
                      d + o_ws, s);
  if (rc) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  std::vector<int32_t> st(n);
  HIP_TRY(ctx, hipMemcpyAsync(st.data(), d + o_st, 4 * n, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  memcpy(status, st.data(), 4 * n);
  return DAGPU_OK;
}

size_t dagpu_nmt_verify_namespace_workspace_size(size_t n, size_t n_leaves) {
  // as dagpu_nmt_verify_workspace_size with 9-word descriptors; an absence
  // proof has one record and no leaf, so every proof may add one
  return pv_nmt_meta_bytes(n, kPvDescNmtNs) + (size_t)kRecNmt * (2 * (n_leaves + n) + 3 * n) + 256;
}

int dagpu_nmt_verify_namespace_batch_device(dagpu_ctx* ctx, size_t n, const int64_t* desc,
                                            const uint8_t* d_namespaces, size_t n_ns, const uint8_t* d_leaves,
                                            size_t n_leaves, size_t leaf_len, const uint8_t* d_nodes, size_t n_nodes,
                                            const uint8_t* d_leaf_hashes, size_t n_leaf_hashes,
                                            const uint8_t* d_roots, size_t n_roots, int32_t* d_status,
                                            void* d_workspace, void* stream) {
  if (!ctx) return DAGPU_ERR_ARG;
  if (n == 0) return DAGPU_OK;
  if (!desc || !d_status || !d_workspace || (((uintptr_t)d_workspace) & 15) != 0 || (n_ns && !d_namespaces) ||
      (n_leaves && leaf_len && !d_leaves) || (n_nodes && !d_nodes) || (n_leaf_hashes && !d_leaf_hashes) ||
      (n_roots && !d_roots))
    return set_err(ctx, DAGPU_ERR_ARG, "dagpu_nmt_verify_namespace_batch_device: null or misaligned buffer");
  PvNmtPlan plan;
  int rc = pv_check_nmt(ctx, n, desc, n_ns, n_leaves, n_nodes, n_roots, &plan, kPvDescNmtNs, n_leaf_hashes);
  if (rc) return rc;
  return pv_nmt_enqueue(ctx, n, plan, d_namespaces, d_leaves, leaf_len, d_nodes, d_roots, d_status,
                        (uint8_t*)d_workspace, (hipStream_t)stream, kPvDescNmtNs, d_leaf_hashes);
}

int dagpu_nmt_verify_namespace_batch(dagpu_ctx* ctx, size_t n, const int64_t* desc, const uint8_t* namespaces,
                                     size_t n_ns, const uint8_t* leaves, size_t n_leaves, size_t leaf_len,
                                     const uint8_t* nodes, size_t n_nodes, const uint8_t* leaf_hashes,
                                     size_t n_leaf_hashes, const uint8_t* roots, size_t n_roots, int32_t* status) {
  if (!ctx) return DAGPU_ERR_ARG;
  if (n == 0) return DAGPU_OK;
  if (!desc || !status || (n_ns && !namespaces) || (n_leaves && leaf_len && !leaves) || (n_nodes && !nodes) ||
      (n_leaf_hashes && !leaf_hashes) || (n_roots && !roots))
    return set_err(ctx, DAGPU_ERR_ARG, "dagpu_nmt_verify_namespace_batch: null buffer");
  PvNmtPlan plan;
  int rc = pv_check_nmt(ctx, n, desc, n_ns, n_leaves, n_nodes, n_roots, &plan, kPvDescNmtNs, n_leaf_hashes);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  (void)hipSetDevice(ctx->device);
  hipStream_t s = ctx->stream;
  const size_t b_ns = n_ns * kNsSize, b_lv = n_leaves * leaf_len, b_nd = n_nodes * kNodeSize,
               b_lh = n_leaf_hashes * kNodeSize, b_rt = n_roots * kNodeSize;
  const size_t o_ns = 0, o_lv = o_ns + ws_align256(b_ns), o_nd = o_lv + ws_align256(b_lv), o_lh = o_nd + ws_align256(b_nd),
               o_rt = o_lh + ws_align256(b_lh), o_st = o_rt + ws_align256(b_rt), o_ws = o_st + ws_align256(4 * n);
  const size_t ws = pv_nmt_meta_bytes(n, kPvDescNmtNs) + (size_t)kRecNmt * (size_t)(plan.n_records + plan.n_stack) + 256;
  PvScratch m;
  HIP_TRY(ctx, hipMalloc(&m.p, o_ws + ws));
  uint8_t* d = (uint8_t*)m.p;
  if (b_ns) HIP_TRY(ctx, hipMemcpyAsync(d + o_ns, namespaces, b_ns, hipMemcpyHostToDevice, s));
  if (b_lv) HIP_TRY(ctx, hipMemcpyAsync(d + o_lv, leaves, b_lv, hipMemcpyHostToDevice, s));
  if (b_nd) HIP_TRY(ctx, hipMemcpyAsync(d + o_nd, nodes, b_nd, hipMemcpyHostToDevice, s));
  if (b_lh) HIP_TRY(ctx, hipMemcpyAsync(d + o_lh, leaf_hashes, b_lh, hipMemcpyHostToDevice, s));
  if (b_rt) HIP_TRY(ctx, hipMemcpyAsync(d + o_rt, roots, b_rt, hipMemcpyHostToDevice, s));
  rc = pv_nmt_enqueue(ctx, n, plan, d + o_ns, d + o_lv, leaf_len, d + o_nd, d + o_rt, (int32_t*)(d + o_st),
                      d + o_ws, s, kPvDescNmtNs, d + o_lh);
  if (rc) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  std::vector<int32_t> st(n);
  HIP_TRY(ctx, hipMemcpyAsync(st.data(), d + o_st, 4 * n, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  memcpy(status, st.data(), 4 * n);
  return DAGPU_OK;
}

int dagpu_merkle_verify_batch(dagpu_ctx* ctx, size_t n, const int64_t* desc, const uint8_t* leaves, size_t n_leaves,
                              size_t leaf_len, const uint8_t* leaf_hashes, const uint8_t* aunts, size_t n_aunts,
                              const uint8_t* roots32, size_t n_roots, int32_t* status) {
  if (!ctx) return DAGPU_ERR_ARG;
  if (n == 0) return DAGPU_OK;
  if (!desc || !status || (n_leaves && leaf_len && !leaves) || (n_aunts && !aunts) || (n_roots && !roots32))
    return set_err(ctx, DAGPU_ERR_ARG, "dagpu_merkle_verify_batch: null buffer");
  for (size_t i = 0; i < n; i++) {
    const int64_t* d = desc + i * kPvDescMerkle;
    if (!pv_span_ok(d[3], d[2], n_aunts) || d[4] < 0 || (uint64_t)d[4] >= n_leaves || d[5] < 0 ||
        (uint64_t)d[5] >= n_roots)
      return set_err(ctx, DAGPU_ERR_ARG, "proof descriptor " + std::to_string(i) + " points outside the buffers");
  }
  std::lock_guard<std::mutex> g(ctx->mu);
  (void)hipSetDevice(ctx->device);
  hipStream_t s = ctx->stream;
  const size_t b_ds = n * kPvDescMerkle * sizeof(int64_t), b_lv = n_leaves * leaf_len, b_lh = leaf_hashes ? 32 * n : 0,
               b_au = 32 * n_aunts, b_rt = 32 * n_roots;
  const size_t o_ds = 0, o_lv = o_ds + ws_align256(b_ds), o_lh = o_lv + ws_align256(b_lv), o_au = o_lh + ws_align256(b_lh),
               o_rt = o_au + ws_align256(b_au), o_st = o_rt + ws_align256(b_rt);
  PvScratch m;
  HIP_TRY(ctx, hipMalloc(&m.p, o_st + ws_align256(4 * n)));
  uint8_t* d = (uint8_t*)m.p;
  HIP_TRY(ctx, hipMemcpyAsync(d + o_ds, desc, b_ds, hipMemcpyHostToDevice, s));
  if (b_lv) HIP_TRY(ctx, hipMemcpyAsync(d + o_lv, leaves, b_lv, hipMemcpyHostToDevice, s));
  if (b_lh) HIP_TRY(ctx, hipMemcpyAsync(d + o_lh, leaf_hashes, b_lh, hipMemcpyHostToDevice, s));
  if (b_au) HIP_TRY(ctx, hipMemcpyAsync(d + o_au, aunts, b_au, hipMemcpyHostToDevice, s));
  if (b_rt) HIP_TRY(ctx, hipMemcpyAsync(d + o_rt, roots32, b_rt, hipMemcpyHostToDevice, s));
  PvMerkleArgs a{};
  a.n = (long)n;
  a.desc = (const int64_t*)(d + o_ds);
  a.leaves = d + o_lv;
  a.leaf_len = (long)leaf_len;
  a.leaf_hashes = leaf_hashes ? d + o_lh : nullptr;
  a.aunts = d + o_au;
  a.roots = d + o_rt;
  a.status = (int32_t*)(d + o_st);
  hipError_t e = launch_pv_merkle(a, s);
  std::vector<int32_t> st(n);
  if (e == hipSuccess) e = hipMemcpyAsync(st.data(), d + o_st, 4 * n, hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);  // the uploads read caller memory: always wait
  HIP_TRY(ctx, e);
  HIP_TRY(ctx, e2);
  memcpy(status, st.data(), 4 * n);
  return DAGPU_OK;
}

int dagpu_subtree_width(uint64_t share_count, uint32_t subtree_root_threshold) {
  if (subtree_root_threshold == 0) return DAGPU_ERR_ARG;
  return (int)subtree_width(share_count, subtree_root_threshold);
}

int dagpu_blob_commitments(dagpu_ctx* ctx, size_t nblobs, const uint8_t* namespaces,
                           const uint32_t* share_counts, const uint8_t* shares,
                           uint32_t subtree_root_threshold, uint8_t* commitments) {
  if (!ctx || (nblobs && (!namespaces || !share_counts || !commitments))) return DAGPU_ERR_ARG;
  if (subtree_root_threshold == 0) return set_err(ctx, DAGPU_ERR_ARG, "subtree root threshold must be positive");
  std::lock_guard<std::mutex> g(ctx->mu);
  (void)hipSetDevice(ctx->device);
  // Plan: one NMT per MMR tree (leaf = namespace | share, commitment.go:53-63),
  // then one RFC-6962 tree per blob over its subtree roots (commitment.go:73).
  std::vector<long> tree_sizes, trees_per_blob(nblobs);
  long nshares = 0;
  for (size_t b = 0; b < nblobs; b++) {
    const uint64_t c = share_counts[b];
    if (c == 0) return set_err(ctx, DAGPU_ERR_ARG, "blob has no shares");
    const auto sz = mmr_sizes(c, subtree_width(c, subtree_root_threshold));
    trees_per_blob[b] = (long)sz.size();
    tree_sizes.insert(tree_sizes.end(), sz.begin(), sz.end());
    nshares += (long)c;
  }
  if (nshares && !shares) return DAGPU_ERR_ARG;
  hipStream_t s = ctx->stream;
  // leaves: namespace(29) | share(512) = 541 B, stride 544
  const long llen = kNsSize + kShareSize, stride = round4(llen);
  std::vector<uint8_t> host((size_t)(stride * (nshares > 0 ? nshares : 1)), 0);
  {
    long i = 0;
    for (size_t b = 0; b < nblobs; b++)
      for (uint32_t j = 0; j < share_counts[b]; j++, i++) {
        memcpy(&host[(size_t)(i * stride)], namespaces + b * kNsSize, kNsSize);
        memcpy(&host[(size_t)(i * stride + kNsSize)], shares + (size_t)i * kShareSize, kShareSize);
      }
  }
  HIP_TRY(ctx, ctx->t_leaf_data.ensure(host.size()));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->t_leaf_data.p, host.data(), host.size(), hipMemcpyHostToDevice, s));
  ForestPlan nplan = ForestPlan::ragged_plan(tree_sizes);
  ForestPlan rplan = ForestPlan::ragged_plan(trees_per_blob);
  const long ntrees = (long)tree_sizes.size();
  const long item_stride = 92;  // 90-B subtree roots, 4-B aligned
  const size_t meta_n = nplan.meta.size() + rplan.meta.size();
  HIP_TRY(ctx, ctx->t_leaves.ensure((size_t)(kRecNmt * (nshares + 1))));
  HIP_TRY(ctx, ctx->t_inner.ensure((size_t)(kRecNmt * (nplan.inner_records + 1))));
  HIP_TRY(ctx, ctx->t_meta.ensure(meta_n * sizeof(int64_t) + 16));
  HIP_TRY(ctx, ctx->t_out.ensure((size_t)(item_stride * ntrees + kRecRfc * (ntrees + rplan.inner_records) +
                                          32 * nblobs + 64)));
  HIP_TRY(ctx, ctx->t_status.ensure((size_t)(4 * ntrees + 4)));
  HIP_TRY(ctx, hipMemsetAsync(ctx->t_status.p, 0, (size_t)(4 * ntrees + 4), s));
  ForestLeafArgs la{};
  la.data = (const uint8_t*)ctx->t_leaf_data.p;
  la.data_stride = stride;
  la.dlen = llen;
  la.nleaves = nshares;
  la.pmode = kPfxNone;
  la.rfc = 0;
  la.out = (uint8_t*)ctx->t_leaves.p;
  HIP_TRY(ctx, launch_forest_leaves(la, s));
  uint8_t* items = (uint8_t*)ctx->t_out.p;
  uint8_t* rleaves = items + item_stride * ntrees;
  uint8_t* rinner = rleaves + kRecRfc * ntrees;
  uint8_t* out = rinner + kRecRfc * (rplan.inner_records + 1);
  int64_t* meta = (int64_t*)ctx->t_meta.p;
  HIP_TRY(ctx, forest_enqueue(nplan, (const uint8_t*)ctx->t_leaves.p, (uint8_t*)ctx->t_inner.p, meta, 1, 1, 0,
                              (int32_t*)ctx->t_status.p, items, 0, item_stride, s));
  ForestLeafArgs ra{};
  ra.data = items;
  ra.data_stride = item_stride;
  ra.dlen = kNodeSize;
  ra.nleaves = ntrees;
  ra.pmode = kPfxNone;
  ra.rfc = 1;
  ra.out = rleaves;
  HIP_TRY(ctx, launch_forest_leaves(ra, s));
  HIP_TRY(ctx, forest_enqueue(rplan, rleaves, rinner, meta + nplan.meta.size(), 0, 0, 1, nullptr, out, 0, 0, s));
  std::vector<int32_t> st(ntrees);
  if (nblobs) HIP_TRY(ctx, hipMemcpyAsync(commitments, out, 32 * nblobs, hipMemcpyDeviceToHost, s));
  if (ntrees) HIP_TRY(ctx, hipMemcpyAsync(st.data(), ctx->t_status.p, 4 * ntrees, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  for (long t = 0; t < ntrees; t++)
    if (st[t]) return set_err(ctx, DAGPU_ERR_PUSH_ORDER, "invalid push order");
  return DAGPU_OK;
}

}  // extern "C"
