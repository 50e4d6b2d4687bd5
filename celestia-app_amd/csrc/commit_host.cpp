// commit_host.cpp -- C ABI of the share commitments computed from squares
// resident in HBM (include/dagpu.h):
//   dagpu_square_plan_blobs        the blob table of a checked plan
//   dagpu_blob_commitments_device  inclusion.CreateCommitment
//                                  (pkg/inclusion/commitment.go:19-75) of many
//                                  share ranges of many squares, compared with
//                                  the declared commitments on the device
//                                  (x/blob/types/blob_tx.go:91-100)
// Request checks and tables in commit_layout.hpp, kernels in blob_commit.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/dagpu.h"
#include "commit_layout.hpp"
#include "forest.hpp"
#include "runtime.hpp"
#include "square_write.hpp"

extern "C" {

int dagpu_square_plan_blobs(const uint8_t* plan, size_t plan_bytes, uint32_t* out, size_t cap, size_t* nblob) {
  using namespace dagpu;
  if (!nblob) return set_err(nullptr, DAGPU_ERR_ARG, "null nblob");
  *nblob = 0;
  size_t src_bytes = 0;  // the plan's own: the check then bounds every data range by it
  if (plan && ((uintptr_t)plan & 3) == 0 && plan_bytes >= sizeof(SqHdr)) src_bytes = ((const SqHdr*)plan)->src_bytes;
  const int rc = dagpu_square_plan_check(plan, plan_bytes, src_bytes);
  if (rc != DAGPU_OK) return rc;
  const SqHdr& h = *(const SqHdr*)plan;
  *nblob = h.nblob;
  if (h.nblob > cap || (h.nblob && !out))
    return set_err(nullptr, DAGPU_ERR_ARG,
                   "the plan has " + std::to_string(h.nblob) + " blobs, the output holds " + std::to_string(cap));
  const uint32_t* b = (const uint32_t*)(plan + h.blob_off);
  for (uint32_t i = 0; i < h.nblob; i++)
    for (int j = 0; j < 4; j++) out[4 * i + j] = b[i * kSqBlobWords + 8 + j];
  return DAGPU_OK;
}

size_t dagpu_blob_commitments_workspace_size(uint32_t k, size_t nblobs, size_t nshares_total) {
  (void)k;  // the tables and records scale with the blobs and shares alone
  using namespace dagpu;
  return commit_carve(commit_table_words_max(nblobs, nshares_total), nshares_total, nshares_total).total;
}

int dagpu_blob_commitments_device(dagpu_ctx* ctx, uint32_t k, size_t n, size_t nblobs, const int64_t* blobs,
                                  const uint8_t* d_squares, size_t square_stride, size_t row_pitch,
                                  uint32_t subtree_root_threshold, uint8_t* d_commitments, const uint8_t* d_expected,
                                  int32_t* d_status, int32_t* d_square_status, void* d_workspace, void* stream) {
  using namespace dagpu;
  if (!ctx) return DAGPU_ERR_ARG;
  if (nblobs && (!blobs || !d_squares || !d_commitments || !d_status))
    return set_err(ctx, DAGPU_ERR_ARG, "dagpu_blob_commitments_device: null argument");
  if ((uintptr_t)d_workspace & 15)
    return set_err(ctx, DAGPU_ERR_ARG, "dagpu_blob_commitments_device: d_workspace must be a multiple of 16");
  CommitLayout lay;
  size_t bad = 0;
  const CommitCheck cc = commit_layout(k, n, nblobs, blobs, (uint64_t)(uintptr_t)d_squares, square_stride, row_pitch,
                                       subtree_root_threshold, &lay, &bad);
  if (cc != kCommitOk)
    return set_err(ctx, cc == kCommitWideSquare ? DAGPU_ERR_UNSUPPORTED : DAGPU_ERR_ARG,
                   (bad < nblobs ? "blob " + std::to_string(bad) + ": " : std::string("blob commitments: ")) +
                       commit_check_text(cc));
  hipStream_t s = (hipStream_t)stream;
  if (nblobs == 0) {
    if (d_square_status && n) HIP_TRY(ctx, hipMemsetAsync(d_square_status, 0, 4 * n, s));
    return DAGPU_OK;
  }
  const CommitCarve cv = commit_carve(lay.words.size(), lay.nshares, lay.nsub);
  uint8_t* ws = (uint8_t*)d_workspace;
  void* own = nullptr;
  if (!ws) {
    HIP_TRY(ctx, hipMalloc(&own, cv.total));
    ws = (uint8_t*)own;
  }
  uint32_t log2k = 0;
  while ((1u << log2k) < k) log2k++;
  const uint32_t* t = (const uint32_t*)(ws + cv.o_tables);
  CommitArgs a{};
  a.blob = t + lay.o_blob;
  a.share_pre = t + lay.o_share_pre;
  a.sub_pre = t + lay.o_sub_pre;
  a.sub = t + lay.o_sub;
  a.work = t + lay.o_work;
  a.nblobs = (uint32_t)lay.nblobs;
  a.nshares = (uint32_t)lay.nshares;
  a.nsub = (uint32_t)lay.nsub;
  a.nwork = (uint32_t)lay.nwork;
  a.log2k = log2k;
  a.squares = d_squares;
  a.square_stride = square_stride;
  a.row_pitch = row_pitch;
  a.leaves = ws + cv.o_leaves;
  a.inner = ws + cv.o_inner;
  a.dig0 = ws + cv.o_dig0;
  a.dig1 = ws + cv.o_dig1;
  a.commitments = d_commitments;
  a.expected = d_expected;
  a.status = d_status;
  a.square_status = d_square_status;
  const size_t table_bytes = lay.words.size() * sizeof(uint32_t);
  hipEvent_t up = ev_take(ctx);
  auto run = [&]() -> int {
    if (!up) return set_err(ctx, DAGPU_ERR_DEVICE, "no event for the table upload");
    {
      HIP_TRY(ctx, ctx->commit_stage.ensure(table_bytes));
      memcpy(ctx->commit_stage.p, lay.words.data(), table_bytes);
      HIP_TRY(ctx, hipMemcpyAsync(ws + cv.o_tables, ctx->commit_stage.p, table_bytes, hipMemcpyHostToDevice, s));
      HIP_TRY(ctx, hipEventRecord(up, s));
      HIP_TRY(ctx, hipMemsetAsync(d_status, 0, 4 * nblobs, s));
      if (d_square_status) HIP_TRY(ctx, hipMemsetAsync(d_square_status, 0, 4 * n, s));
      HIP_TRY(ctx, launch_commit_leaves(a, s));
      HIP_TRY(ctx, launch_commit_subtrees(a, s));
      HIP_TRY(ctx, launch_commit_roots(a, s));
      HIP_TRY(ctx, hipEventSynchronize(up));
    }
    return DAGPU_OK;
  };
  int rc;
  {
    // the staging buffer is one per context: hold it until the upload has left it
    std::lock_guard<std::mutex> g(ctx->commit_mu);
    rc = run();
    if (rc != DAGPU_OK) (void)hipStreamSynchronize(s);  // an upload may still read the staging buffer
  }
  if (own) {
    // the kernels read the library's own workspace: wait for them, then free
    const hipError_t e = hipStreamSynchronize(s);
    if (rc == DAGPU_OK && e != hipSuccess) rc = hip_fail(ctx, e, "hipStreamSynchronize");
    (void)hipFree(own);
  }
  if (up) ev_give(ctx, up);
  return rc;
}

}  // extern "C"
