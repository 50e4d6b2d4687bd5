// commit_plan_host.cpp -- C ABI of the commitment check laid out on the device
// and of the verdict (include/dagpu.h):
//   dagpu_commit_plan_device / _host       the tables, counts and blob_base from
//                                          the planner's arena and records
//   dagpu_proposal_check_device            ValidateBlobTx's rules, the layout, the
//                                          tie and the commitments in one enqueue
//   dagpu_proposal_verdict_device / _host  one record per block in
//                                          ProcessProposal's order
// Arithmetic in commit_plan.hpp, kernels in commit_plan.hip, blobtx_check.hip
// and blob_commit.hip (the counted forms).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <new>
#include <string>
#include <vector>

#include "../../include/dagpu.h"
#include "commit_layout.hpp"
#include "commit_plan_launch.hpp"
#include "forest.hpp"
#include "runtime.hpp"

namespace dagpu {

namespace {

// workspace of the layout alone: CpSums[n] | CpSums[n]
struct CpCarve {
  uint64_t sums, base, total;
};
CpCarve cp_carve(uint64_t n) {
  CpCarve c;
  c.sums = 0;
  c.base = commit_align256(n * sizeof(CpSums));
  c.total = c.base + commit_align256(n * sizeof(CpSums));
  return c;
}

// workspace of the check: bt_carve | the table image | cp_carve | commit_carve at capacity
struct PcCarve {
  uint64_t bt, tables, cp, commit, total;
  CommitCarve cv;
};
PcCarve pc_carve(uint32_t k, uint64_t n, uint64_t ntx_total) {
  const uint64_t cap = cp_cap_items(k, n);
  PcCarve c;
  c.bt = 0;
  c.tables = commit_align256(bt_carve(n, ntx_total).total);
  c.cp = c.tables + commit_align256(4 * cp_cap_table_words(k, n));
  c.commit = c.cp + cp_carve(n).total;
  c.cv = commit_carve(0, cap, cap);
  c.total = c.commit + c.cv.total;
  return c;
}

// workspace of the verdict: key[n] (uint64) | data hashes n x 32 | square sizes n x 4
struct PvCarve {
  uint64_t key, hashes, sizes, total;
};
PvCarve pv_carve(uint64_t n) {
  PvCarve c;
  c.key = 0;
  c.hashes = sp_up16(n * 8);
  c.sizes = c.hashes + n * 32;
  c.total = sp_up16(c.sizes + n * 4);
  return c;
}

// k, threshold and the batch's size; 0 or the error code
int cp_check_width(dagpu_ctx* ctx, const char* who, uint32_t k, size_t n, uint32_t threshold) {
  const std::string w(who);
  if (k == 0 || (k & (k - 1)) != 0) return set_err(ctx, DAGPU_ERR_ARG, w + ": square width must be a power of two");
  if (k > kCommitMaxWidth) return set_err(ctx, DAGPU_ERR_UNSUPPORTED, w + ": square width above 1024 is not supported");
  if (threshold == 0) return set_err(ctx, DAGPU_ERR_ARG, w + ": subtree root threshold must be positive");
  if (n >= ((size_t)1 << 24)) return set_err(ctx, DAGPU_ERR_ARG, w + ": more than 2^24 blocks in one call");
  if (cp_cap_items(k, n) >= ((uint64_t)1 << 31))
    return set_err(ctx, DAGPU_ERR_UNSUPPORTED, w + ": n * k * k must stay below 2^31 shares");
  return DAGPU_OK;
}

// The grid cap of the counted kernels, a fixed multiple of the CU count.
// Workgroups of 256 lanes, one item per lane: 8 per CU fill every wave slot.
// Workgroups of one wave, one blob or subtree per round: 128 per CU, several
// times what is resident, so that the dispatcher evens out rounds of unequal
// length as it does for the uncounted kernels' one workgroup per item (with 8
// and 32 per CU the root kernel of 128,000 blobs took 2.97 and 2.19 ms against
// 1.83 ms uncounted; profiles/process_blocks_device.log has the final figures).
constexpr uint32_t kGroupsPerCu = 8, kWaveGroupsPerCu = 128;
uint32_t counted_grid_cap(dagpu_ctx* ctx, uint32_t groups_per_cu) {
  static std::atomic<int> cus_of[64];
  const int d = ctx->device >= 0 && ctx->device < 64 ? ctx->device : 0;
  int cus = cus_of[d].load(std::memory_order_relaxed);
  if (cus <= 0) {
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || cus <= 0)
      cus = 256;
    cus_of[d].store(cus, std::memory_order_relaxed);
  }
  uint32_t cap = groups_per_cu * (uint32_t)cus;
#if defined(DAGPU_TEST_HOOKS)
  // the test build only: a small grid sends every workgroup round its stride loop
  if (const char* e = getenv("DAGPU_TEST_COMMIT_GRID")) {
    const long v = atol(e);
    if (v > 0 && (uint64_t)v < cap) cap = (uint32_t)v;
  }
#endif
  return cap;
}

CpArgs cp_args(uint8_t* ws, uint32_t k, size_t n, const uint8_t* plans, size_t plans_cap, const void* records,
               uint32_t threshold, uint32_t* tables, uint32_t* counts, uint64_t* blob_base) {
  const CpCarve c = cp_carve(n);
  CpArgs a;
  a.arena = plans;
  a.arena_cap = plans_cap;
  a.rec = (const SpRecord*)records;
  a.n = (uint32_t)n;
  a.k = k;
  a.threshold = threshold;
  a.sums = (CpSums*)(ws + c.sums);
  a.base = (CpSums*)(ws + c.base);
  a.tables = tables;
  a.counts = counts;
  a.blob_base = blob_base;
  return a;
}

int cp_request(dagpu_ctx* ctx, uint32_t k, size_t n, const void* plans, const void* records, uint32_t threshold,
               const void* tables, const void* counts, const void* blob_base) {
  const int rc = cp_check_width(ctx, "commit plan", k, n, threshold);
  if (rc != DAGPU_OK) return rc;
  if (!plans || !records || !tables || !counts || !blob_base)
    return set_err(ctx, DAGPU_ERR_ARG, "commit plan: null argument");
  if (((uintptr_t)plans | (uintptr_t)records | (uintptr_t)tables | (uintptr_t)counts) & 15 || (uintptr_t)blob_base & 7)
    return set_err(ctx, DAGPU_ERR_ARG,
                   "commit plan: plans, records, tables and counts must be 16-byte and blob_base 8-byte aligned");
  return DAGPU_OK;
}

}  // namespace

}  // namespace dagpu

extern "C" {

size_t dagpu_commit_plan_table_words(uint32_t k, size_t n) { return (size_t)dagpu::cp_cap_table_words(k, n); }

size_t dagpu_commit_plan_workspace_size(uint32_t k, size_t n) {
  (void)k;
  return (size_t)dagpu::cp_carve(n).total;
}

int dagpu_commit_plan_device(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* d_plans, size_t plans_cap,
                             const void* d_records, uint32_t subtree_root_threshold, uint32_t* d_tables,
                             uint32_t* d_counts, uint64_t* d_blob_base, void* d_workspace, void* stream) {
  using namespace dagpu;
  if (!ctx) return DAGPU_ERR_ARG;
  if (n == 0) return DAGPU_OK;
  const int rc0 = cp_request(ctx, k, n, d_plans, d_records, subtree_root_threshold, d_tables, d_counts, d_blob_base);
  if (rc0 != DAGPU_OK) return rc0;
  if ((uintptr_t)d_workspace & 15) return set_err(ctx, DAGPU_ERR_ARG, "commit plan: d_workspace must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)d_workspace;
  void* own = nullptr;
  if (!ws) {
    HIP_TRY(ctx, hipMalloc(&own, cp_carve(n).total));
    ws = (uint8_t*)own;
  }
  const CpArgs a =
      cp_args(ws, k, n, d_plans, plans_cap, d_records, subtree_root_threshold, d_tables, d_counts, d_blob_base);
  int rc = DAGPU_OK;
  const hipError_t e = launch_commit_plan(a, s);
  if (e != hipSuccess) rc = hip_fail(ctx, e, "commit plan launch");
  if (own) {
    const hipError_t e2 = hipStreamSynchronize(s);
    if (rc == DAGPU_OK && e2 != hipSuccess) rc = hip_fail(ctx, e2, "hipStreamSynchronize");
    (void)hipFree(own);
  }
  return rc;
}

int dagpu_commit_plan_host(uint32_t k, size_t n, const uint8_t* plans, size_t plans_cap, const void* records,
                           uint32_t subtree_root_threshold, uint32_t* tables, uint32_t* counts, uint64_t* blob_base) {
  using namespace dagpu;
  if (n == 0) return DAGPU_OK;
  const int rc = cp_request(nullptr, k, n, plans, records, subtree_root_threshold, tables, counts, blob_base);
  if (rc != DAGPU_OK) return rc;
  try {
    std::vector<uint64_t> ws(cp_carve(n).total / 8 + 1);
    cp_layout_host(cp_args((uint8_t*)ws.data(), k, n, plans, plans_cap, records, subtree_root_threshold, tables,
                           counts, blob_base));
  } catch (const std::bad_alloc&) {
    return set_err(nullptr, DAGPU_ERR_ARG, "out of host memory");
  }
  return DAGPU_OK;
}

size_t dagpu_proposal_check_workspace_size(uint32_t k, size_t n, size_t ntx_total) {
  return (size_t)dagpu::pc_carve(k, n, ntx_total).total;
}

int dagpu_proposal_check_device(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* d_src, const size_t* src_offs,
                                size_t src_bytes, const uint32_t* ntx, const uint64_t* tx_lens,
                                const uint8_t* d_plans, size_t plans_cap, const void* d_records,
                                const uint8_t* d_squares, size_t square_stride, size_t row_pitch,
                                uint32_t subtree_root_threshold, uint32_t* d_tx_status, uint32_t* d_block_status,
                                uint8_t* d_expected, uint8_t* d_commitments, int32_t* d_blob_status,
                                uint32_t* d_row_tx, int32_t* d_square_status, uint32_t* d_counts,
                                uint64_t* d_blob_base, void* d_workspace, void* stream) {
  using namespace dagpu;
  if (!ctx) return DAGPU_ERR_ARG;
  if (n == 0) return DAGPU_OK;
  const int rcw = cp_check_width(ctx, "proposal check", k, n, subtree_root_threshold);
  if (rcw != DAGPU_OK) return rcw;
  if (!d_plans || !d_records || !d_squares || !d_expected || !d_commitments || !d_blob_status || !d_row_tx ||
      !d_square_status || !d_counts || !d_blob_base)
    return set_err(ctx, DAGPU_ERR_ARG, "proposal check: null argument");
  if (row_pitch < (size_t)k * 512) return set_err(ctx, DAGPU_ERR_ARG, "proposal check: row_pitch below k * 512");
  if (((uintptr_t)d_squares | square_stride | row_pitch) & 15)
    return set_err(ctx, DAGPU_ERR_ARG, "proposal check: d_squares, square_stride and row_pitch must be multiples of 16");
  if (((uintptr_t)d_plans | (uintptr_t)d_records | (uintptr_t)d_counts | (uintptr_t)d_workspace |
       (uintptr_t)d_expected | (uintptr_t)d_commitments) & 15 ||
      ((uintptr_t)d_blob_base | (uintptr_t)d_row_tx) & 7 || ((uintptr_t)d_blob_status | (uintptr_t)d_square_status) & 3)
    return set_err(ctx, DAGPU_ERR_ARG,
                   "proposal check: d_plans, d_records, d_counts, d_expected, d_commitments and d_workspace must be "
                   "16-byte, d_blob_base and d_row_tx 8-byte, the status arrays 4-byte aligned");
  std::vector<uint8_t> up;
  uint64_t ntx_total = 0, nrows = 0;
  const int rc0 = bt_request(ctx, n, d_src, src_offs, src_bytes, ntx, tx_lens, d_plans, d_records, nullptr,
                             d_tx_status, d_block_status, d_expected, up, ntx_total, nrows);
  if (rc0 != DAGPU_OK) return rc0;
  hipStream_t s = (hipStream_t)stream;
  const PcCarve c = pc_carve(k, n, ntx_total);
  const BtCarve bc = bt_carve(n, ntx_total);
  const uint64_t cap = cp_cap_items(k, n);
  uint8_t* ws = (uint8_t*)d_workspace;
  void* own = nullptr;
  if (!ws) {
    HIP_TRY(ctx, hipMalloc(&own, c.total));
    ws = (uint8_t*)own;
  }
  BtArgs bt = bt_args(ws + c.bt, d_src, n, ntx_total, 0, d_plans, plans_cap, d_records, d_tx_status, d_block_status,
                      d_expected);
  bt.blob_base = d_blob_base;  // the layout's, in device memory
  uint32_t* tables = (uint32_t*)(ws + c.tables);
  const CpArgs cp = cp_args(ws + c.cp, k, n, d_plans, plans_cap, d_records, subtree_root_threshold, tables, d_counts,
                            d_blob_base);
  uint32_t log2k = 0;
  while ((1u << log2k) < k) log2k++;
  CommitCounted cc{};
  cc.tables = tables;
  cc.counts = d_counts;
  cc.a.log2k = log2k;
  cc.a.squares = d_squares;
  cc.a.square_stride = square_stride;
  cc.a.row_pitch = row_pitch;
  cc.a.leaves = ws + c.commit + c.cv.o_leaves;
  cc.a.inner = ws + c.commit + c.cv.o_inner;
  cc.a.dig0 = ws + c.commit + c.cv.o_dig0;
  cc.a.dig1 = ws + c.commit + c.cv.o_dig1;
  cc.a.commitments = d_commitments;
  cc.a.expected = d_expected;
  cc.a.status = d_blob_status;
  cc.a.square_status = d_square_status;
  const uint32_t grid_cap = counted_grid_cap(ctx, kGroupsPerCu),
                 wave_grid_cap = counted_grid_cap(ctx, kWaveGroupsPerCu);
  hipEvent_t done = ev_take(ctx);
  auto run = [&]() -> int {
    if (!done) return set_err(ctx, DAGPU_ERR_DEVICE, "no event for the upload");
    HIP_TRY(ctx, ctx->commit_stage.ensure(up.size()));
    memcpy(ctx->commit_stage.p, up.data(), up.size());
    HIP_TRY(ctx, hipMemsetAsync(ws + c.bt, 0xFF, n * 8, s));
    HIP_TRY(ctx, hipMemcpyAsync(ws + c.bt + bc.blk, ctx->commit_stage.p, up.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipEventRecord(done, s));
    HIP_TRY(ctx, hipMemsetAsync(d_blob_status, 0, 4 * cap, s));
    HIP_TRY(ctx, hipMemsetAsync(d_square_status, 0, 4 * n, s));
    HIP_TRY(ctx, launch_bt_validate(bt, s));
    HIP_TRY(ctx, launch_bt_finish(bt, s));
    HIP_TRY(ctx, launch_commit_plan(cp, s));
    HIP_TRY(ctx, launch_bt_tie_counted(bt, d_row_tx, cap, grid_cap, s));
    HIP_TRY(ctx, launch_commit_leaves_counted(cc, cap, grid_cap, s));
    HIP_TRY(ctx, launch_commit_subtrees_counted(cc, cap / 2, wave_grid_cap, s));
    HIP_TRY(ctx, launch_commit_roots_counted(cc, cap, wave_grid_cap, s));
    // the upload reads the context's staging buffer: hold it until the copy (not the kernels) has passed
    HIP_TRY(ctx, hipEventSynchronize(done));
    return DAGPU_OK;
  };
  int rc;
  {
    std::lock_guard<std::mutex> g(ctx->commit_mu);
    rc = run();
    if (rc != DAGPU_OK) (void)hipStreamSynchronize(s);
  }
  if (own) {
    const hipError_t e = hipStreamSynchronize(s);
    if (rc == DAGPU_OK && e != hipSuccess) rc = hip_fail(ctx, e, "hipStreamSynchronize");
    (void)hipFree(own);
  }
  if (done) ev_give(ctx, done);
  return rc;
}

size_t dagpu_proposal_verdict_workspace_size(uint32_t k, size_t n, size_t ntx_total) {
  (void)k;
  (void)ntx_total;
  return (size_t)dagpu::pv_carve(n).total;
}

}  // extern "C"

namespace dagpu {
namespace {

int pv_request(dagpu_ctx* ctx, uint32_t k, size_t n, const void* records, const void* block_status,
               const void* blob_status, const void* row_tx, const void* blob_base, const void* verdicts) {
  const int rc = cp_check_width(ctx, "proposal verdict", k, n, 1);
  if (rc != DAGPU_OK) return rc;
  if (!records || !block_status || !blob_status || !row_tx || !blob_base || !verdicts)
    return set_err(ctx, DAGPU_ERR_ARG, "proposal verdict: null argument");
  if (((uintptr_t)records | (uintptr_t)verdicts) & 15 ||
      ((uintptr_t)block_status | (uintptr_t)row_tx | (uintptr_t)blob_base) & 7 || (uintptr_t)blob_status & 3)
    return set_err(ctx, DAGPU_ERR_ARG,
                   "proposal verdict: records and verdicts must be 16-byte, block_status, row_tx and blob_base 8-byte, "
                   "blob_status 4-byte aligned");
  return DAGPU_OK;
}

}  // namespace
}  // namespace dagpu

extern "C" {

int dagpu_proposal_verdict_device(dagpu_ctx* ctx, uint32_t k, size_t n, const void* d_records,
                                  const uint32_t* d_block_status, const int32_t* d_blob_status,
                                  const uint32_t* d_row_tx, const uint64_t* d_blob_base,
                                  const int32_t* d_extend_status, const uint8_t* d_dah, const uint8_t* data_hashes,
                                  const uint32_t* square_sizes, uint32_t* d_verdicts, void* d_workspace,
                                  void* stream) {
  using namespace dagpu;
  if (!ctx) return DAGPU_ERR_ARG;
  if (n == 0) return DAGPU_OK;
  const int rc0 = pv_request(ctx, k, n, d_records, d_block_status, d_blob_status, d_row_tx, d_blob_base, d_verdicts);
  if (rc0 != DAGPU_OK) return rc0;
  if (data_hashes && !d_dah) return set_err(ctx, DAGPU_ERR_ARG, "proposal verdict: data_hashes without d_dah");
  if ((uintptr_t)d_workspace & 15)
    return set_err(ctx, DAGPU_ERR_ARG, "proposal verdict: d_workspace must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const PvCarve c = pv_carve(n);
  uint8_t* ws = (uint8_t*)d_workspace;
  void* own = nullptr;
  if (!ws) {
    HIP_TRY(ctx, hipMalloc(&own, c.total));
    ws = (uint8_t*)own;
  }
  PvArgs a;
  a.rec = (const SpRecord*)d_records;
  a.block_status = d_block_status;
  a.blob_status = d_blob_status;
  a.row_tx = d_row_tx;
  a.blob_base = d_blob_base;
  a.extend_status = d_extend_status;
  a.dah = d_dah;
  a.hashes = data_hashes ? ws + c.hashes : nullptr;
  a.sizes = square_sizes ? (const uint32_t*)(ws + c.sizes) : nullptr;
  a.key = (unsigned long long*)(ws + c.key);
  a.verdicts = d_verdicts;
  a.n = (uint32_t)n;
  a.k = k;
  const bool upload = data_hashes || square_sizes;
  const uint32_t grid_cap = counted_grid_cap(ctx, kGroupsPerCu);
  hipEvent_t done = upload ? ev_take(ctx) : nullptr;
  auto run = [&]() -> int {
    HIP_TRY(ctx, hipMemsetAsync(ws + c.key, 0xFF, n * 8, s));
    if (upload) {
      if (!done) return set_err(ctx, DAGPU_ERR_DEVICE, "no event for the upload");
      // hashes | sizes side by side, as the workspace holds them: one copy
      HIP_TRY(ctx, ctx->commit_stage.ensure(n * 36));
      uint8_t* st = (uint8_t*)ctx->commit_stage.p;
      if (data_hashes) memcpy(st, data_hashes, n * 32);
      if (square_sizes) memcpy(st + n * 32, square_sizes, n * 4);
      const size_t from = data_hashes ? 0 : n * 32, to = square_sizes ? n * 36 : n * 32;
      HIP_TRY(ctx, hipMemcpyAsync(ws + c.hashes + from, st + from, to - from, hipMemcpyHostToDevice, s));
      HIP_TRY(ctx, hipEventRecord(done, s));
    }
    HIP_TRY(ctx, launch_verdict(a, cp_cap_items(k, n), grid_cap, s));
    if (upload) HIP_TRY(ctx, hipEventSynchronize(done));
    return DAGPU_OK;
  };
  int rc;
  {
    std::unique_lock<std::mutex> g(ctx->commit_mu, std::defer_lock);
    if (upload) g.lock();
    rc = run();
    if (rc != DAGPU_OK) (void)hipStreamSynchronize(s);
  }
  if (own) {
    const hipError_t e = hipStreamSynchronize(s);
    if (rc == DAGPU_OK && e != hipSuccess) rc = hip_fail(ctx, e, "hipStreamSynchronize");
    (void)hipFree(own);
  }
  if (done) ev_give(ctx, done);
  return rc;
}

int dagpu_proposal_verdict_host(uint32_t k, size_t n, const void* records, const uint32_t* block_status,
                                const int32_t* blob_status, const uint32_t* row_tx, const uint64_t* blob_base,
                                const int32_t* extend_status, const uint8_t* dah, const uint8_t* data_hashes,
                                const uint32_t* square_sizes, uint32_t* verdicts) {
  using namespace dagpu;
  if (n == 0) return DAGPU_OK;
  const int rc = pv_request(nullptr, k, n, records, block_status, blob_status, row_tx, blob_base, verdicts);
  if (rc != DAGPU_OK) return rc;
  if (data_hashes && !dah) return set_err(nullptr, DAGPU_ERR_ARG, "proposal verdict: data_hashes without dah");
  try {
    std::vector<unsigned long long> key(n, kPvNoKey);
    PvArgs a;
    a.rec = (const SpRecord*)records;
    a.block_status = block_status;
    a.blob_status = blob_status;
    a.row_tx = row_tx;
    a.blob_base = blob_base;
    a.extend_status = extend_status;
    a.dah = dah;
    a.hashes = data_hashes;
    a.sizes = square_sizes;
    a.key = key.data();
    a.verdicts = verdicts;
    a.n = (uint32_t)n;
    a.k = k;
    pv_host(a);
  } catch (const std::bad_alloc&) {
    return set_err(nullptr, DAGPU_ERR_ARG, "out of host memory");
  }
  return DAGPU_OK;
}

}  // extern "C"
