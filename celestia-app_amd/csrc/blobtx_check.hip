// blobtx_check.hip -- ValidateBlobTx's stateless rules over the txs of n blocks
// resident in HBM (dagpu_blob_tx_validate_device, include/dagpu.h), and the
// table of declared commitments dagpu_blob_commitments_device compares against.
//
//   bt_validate  one lane per tx of the whole batch: bt_check_tx walks the tx
//                where it lies (byte loads of the envelope and the inner tx;
//                blob data is skipped by length), stores the tx's word and
//                where its MsgPayForBlobs lies, and folds a failing word into
//                its block's lowest (tx index << 32 | word) with one 64-bit
//                atomic min: the lowest tx index wins whatever the scheduling.
//   bt_finish    one lane per block: the two words of d_block_status.
//   bt_tie       one lane per row of the expected table: two binary searches
//                (the row's block, the tx that holds the plan blob's data_off)
//                and a walk of that one tx; 32 bytes copied, or zeros.
// The arithmetic is blobtx_check.hpp, shared with dagpu_blob_tx_validate_host
// (blobtx_host.cpp).  The work is divergent and small, like sp_classify: about
// 300 B of inner tx per lane.  Reads of src stay inside the tx a lane walks
// (sp_next_field checks every length against the end first); reads of the arena
// stay inside the plan its record names, checked against plans_cap; stores go
// to the lane's own tx, block or row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "blobtx_check.hpp"
#include "runtime.hpp"

namespace dagpu {

__global__ __launch_bounds__(256) void bt_validate(BtArgs a) {
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.ntx_total) return;
  uint32_t blk;
  const uint64_t key = bt_validate_tx(a, g, blk);
  if (key != ~(uint64_t)0) atomicMin(&a.lowest[blk], (unsigned long long)key);
}

__global__ __launch_bounds__(256) void bt_finish(BtArgs a) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.n) bt_finish_block(a, i);
}

__global__ __launch_bounds__(256) void bt_tie(BtArgs a) {
  const uint64_t row = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (row < a.nrows) bt_tie_row(a, row);
}

// for dagpu_proposal_check_device (commit_plan_host.cpp)
hipError_t launch_bt_validate(const BtArgs& a, hipStream_t s) {
  if (a.ntx_total == 0) return hipSuccess;
  hipLaunchKernelGGL(bt_validate, dim3((unsigned)((a.ntx_total + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_bt_finish(const BtArgs& a, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(bt_finish, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dagpu

extern "C" {

int dagpu_blob_tx_validate_device(dagpu_ctx* ctx, size_t n, const uint8_t* d_src, const size_t* src_offs,
                                  size_t src_bytes, const uint32_t* ntx, const uint64_t* tx_lens,
                                  const uint8_t* d_plans, size_t plans_cap, const void* d_records,
                                  const uint64_t* blob_base, uint32_t* d_tx_status, uint32_t* d_block_status,
                                  uint8_t* d_expected, void* d_workspace, void* stream) {
  using namespace dagpu;
  if (!ctx) return DAGPU_ERR_ARG;
  if (n == 0) return DAGPU_OK;
  if ((uintptr_t)d_workspace & 15) return set_err(ctx, DAGPU_ERR_ARG, "d_workspace must be 16-byte aligned");
  std::vector<uint8_t> up;
  uint64_t ntx_total = 0, nrows = 0;
  const int rc0 = bt_request(ctx, n, d_src, src_offs, src_bytes, ntx, tx_lens, d_plans, d_records, blob_base,
                             d_tx_status, d_block_status, d_expected, up, ntx_total, nrows);
  if (rc0 != DAGPU_OK) return rc0;
  hipStream_t s = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)d_workspace;
  void* own = nullptr;
  const BtCarve c = bt_carve(n, ntx_total);
  if (!ws) {
    HIP_TRY(ctx, hipMalloc(&own, c.total));
    ws = (uint8_t*)own;
  }
  const BtArgs a = bt_args(ws, d_src, n, ntx_total, nrows, d_plans, plans_cap, d_records, d_tx_status, d_block_status,
                           d_expected);
  hipEvent_t done = ev_take(ctx);
  auto run = [&]() -> int {
    if (!done) return set_err(ctx, DAGPU_ERR_DEVICE, "no event for the upload");
    HIP_TRY(ctx, hipMemsetAsync(ws, 0xFF, n * 8, s));
    HIP_TRY(ctx, hipMemcpyAsync(ws + c.blk, up.data(), up.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipEventRecord(done, s));
    if (ntx_total) {
      hipLaunchKernelGGL(bt_validate, dim3((unsigned)((ntx_total + 255) / 256)), dim3(256), 0, s, a);
      HIP_TRY(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(bt_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    HIP_TRY(ctx, hipGetLastError());
    if (nrows) {
      hipLaunchKernelGGL(bt_tie, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, s, a);
      HIP_TRY(ctx, hipGetLastError());
    }
    // the upload reads this frame's vector: wait until it (not the kernels) has passed
    HIP_TRY(ctx, hipEventSynchronize(done));
    return DAGPU_OK;
  };
  int rc = run();
  if (own) {
    const hipError_t e = hipStreamSynchronize(s);
    if (rc == DAGPU_OK && e != hipSuccess) rc = hip_fail(ctx, e, "hipStreamSynchronize");
    (void)hipFree(own);
  } else if (rc != DAGPU_OK) {
    (void)hipStreamSynchronize(s);
  }
  if (done) ev_give(ctx, done);
  return rc;
}

}  // extern "C"
