// blobtx_host.cpp -- the host side of dagpu_blob_tx_validate_* (include/dagpu.h):
// the request checks both executors share, the per-tx word for one buffer
// (dagpu_blob_tx_check) and dagpu_blob_tx_validate_host, which runs the
// functions of blobtx_check.hpp that the kernels of blobtx_check.hip run, as
// loops over host memory.  Needs no context and no device.
#include <new>
#include <string>
#include <vector>

#include "blobtx_check.hpp"
#include "runtime.hpp"

namespace dagpu {

int bt_request(dagpu_ctx* ctx, size_t n, const void* src, const size_t* src_offs, size_t src_bytes, const uint32_t* ntx,
               const uint64_t* tx_lens, const void* plans, const void* records, const uint64_t* blob_base,
               const void* tx_status, const void* block_status, const void* expected, std::vector<uint8_t>& up,
               uint64_t& ntx_total, uint64_t& nrows) {
  if (!src_offs || !ntx || !tx_status || !block_status) return set_err(ctx, DAGPU_ERR_ARG, "null argument");
  if (n >= ((size_t)1 << 24)) return set_err(ctx, DAGPU_ERR_ARG, "more than 2^24 blocks in one call");
  if (((uintptr_t)tx_status & 3) || ((uintptr_t)block_status & 7))
    return set_err(ctx, DAGPU_ERR_ARG, "d_tx_status must be 4-byte and d_block_status 8-byte aligned");
  nrows = 0;
  if (blob_base) {
    if (blob_base[0] != 0) return set_err(ctx, DAGPU_ERR_ARG, "blob_base must start at 0");
    for (size_t i = 0; i < n; i++)
      if (blob_base[i] > blob_base[i + 1])
        return set_err(ctx, DAGPU_ERR_ARG, "blob_base must ascend (block " + std::to_string(i) + ")");
    nrows = blob_base[n];
    if (nrows >= ((uint64_t)1 << 32)) return set_err(ctx, DAGPU_ERR_UNSUPPORTED, "more than 2^32 blobs in one call");
    if (nrows && (!plans || !records || !expected))
      return set_err(ctx, DAGPU_ERR_ARG, "null d_plans, d_records or d_expected with blobs to tie");
    if ((uintptr_t)plans & 15 || (uintptr_t)records & 15)
      return set_err(ctx, DAGPU_ERR_ARG, "d_plans and d_records must be 16-byte aligned");
  }
  const int rc = sp_tables(ctx, n, src, src_offs, src_bytes, ntx, tx_lens, kSpMaxWidth, up, ntx_total);
  if (rc != DAGPU_OK) return rc;
  const size_t at = up.size();
  up.resize(at + (n + 1) * 8, 0);
  if (blob_base) memcpy(up.data() + at, blob_base, (n + 1) * 8);
  return DAGPU_OK;
}

}  // namespace dagpu

extern "C" {

size_t dagpu_blob_tx_validate_workspace_size(size_t n, size_t ntx_total, size_t nblobs_total) {
  (void)nblobs_total;  // a row of the expected table needs no table of its own
  return (size_t)dagpu::bt_carve(n, ntx_total).total;
}

uint32_t dagpu_blob_tx_check(const uint8_t* tx, size_t n) {
  if (n >= dagpu::kSqLitFlag || (n && !tx)) return dagpu::kBtOk;  // no block holds such a tx
  return dagpu::bt_check_tx(tx, (uint32_t)n, nullptr);
}

int dagpu_blob_tx_validate_host(size_t n, const uint8_t* src, const size_t* src_offs, size_t src_bytes,
                                const uint32_t* ntx, const uint64_t* tx_lens, const uint8_t* plans, size_t plans_cap,
                                const void* records, const uint64_t* blob_base, uint32_t* tx_status,
                                uint32_t* block_status, uint8_t* expected) {
  using namespace dagpu;
  if (n == 0) return DAGPU_OK;
  std::vector<uint8_t> up;
  uint64_t ntx_total = 0, nrows = 0;
  const int rc = bt_request(nullptr, n, src, src_offs, src_bytes, ntx, tx_lens, plans, records, blob_base, tx_status,
                            block_status, expected, up, ntx_total, nrows);
  if (rc != DAGPU_OK) return rc;
  try {
    const BtCarve c = bt_carve(n, ntx_total);
    std::vector<uint64_t> ws(c.total / 8 + 1);
    uint8_t* w = (uint8_t*)ws.data();
    memset(w, 0xFF, n * 8);
    memcpy(w + c.blk, up.data(), up.size());
    const BtArgs a = bt_args(w, src, n, ntx_total, nrows, plans, plans_cap, records, tx_status, block_status, expected);
    for (uint64_t g = 0; g < ntx_total; g++) {
      uint32_t blk;
      const uint64_t key = bt_validate_tx(a, g, blk);
      if (key < a.lowest[blk]) a.lowest[blk] = key;
    }
    for (uint32_t i = 0; i < a.n; i++) bt_finish_block(a, i);
    for (uint64_t row = 0; row < nrows; row++) bt_tie_row(a, row);
  } catch (const std::bad_alloc&) {
    return set_err(nullptr, DAGPU_ERR_ARG, "out of host memory");
  }
  return DAGPU_OK;
}

}  // extern "C"
