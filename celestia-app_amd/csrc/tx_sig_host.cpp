// tx_sig_host.cpp -- the host side of dagpu_secp256k1_verify_*, dagpu_tx_signers_*
// and dagpu_tx_sig_verify_* (include/dagpu.h): the request checks both
// executors share and the host executors, which run the functions of
// tx_sig.hpp and secp256k1.hpp that the kernels of tx_sig.hip run, as loops
// over host memory.  Needs no context and no device.
#include <new>
#include <string>
#include <vector>

#include "runtime.hpp"
#include "tx_sig.hpp"

namespace dagpu {

int ts_request(dagpu_ctx* ctx, size_t n, const void* src, const size_t* src_offs, size_t src_bytes, const uint32_t* ntx,
               const uint64_t* tx_lens, bool verify, const uint8_t* chain_id, size_t chain_id_len,
               const void* account_numbers, const void* tx_status, const void* block_status, const void* signers,
               std::vector<uint8_t>& up, uint64_t& ntx_total) {
  if (!src_offs || !ntx || !signers) return set_err(ctx, DAGPU_ERR_ARG, "null argument");
  if (verify && (!tx_status || !block_status)) return set_err(ctx, DAGPU_ERR_ARG, "null argument");
  if (n >= ((size_t)1 << 24)) return set_err(ctx, DAGPU_ERR_ARG, "more than 2^24 blocks in one call");
  if (verify && (((uintptr_t)tx_status | (uintptr_t)block_status) & 3))
    return set_err(ctx, DAGPU_ERR_ARG, "d_tx_status and d_block_status must be 4-byte aligned");
  if ((uintptr_t)signers & 7) return set_err(ctx, DAGPU_ERR_ARG, "d_signers must be 8-byte aligned");
  if (verify && chain_id_len > kTsMaxChainId) return set_err(ctx, DAGPU_ERR_ARG, "chain_id is longer than 64 bytes");
  if (verify && chain_id_len && !chain_id) return set_err(ctx, DAGPU_ERR_ARG, "null chain_id");
  if (verify && ((uintptr_t)account_numbers & 7))
    return set_err(ctx, DAGPU_ERR_ARG, "d_account_numbers must be 8-byte aligned");
  const int rc = sp_tables(ctx, n, src, src_offs, src_bytes, ntx, tx_lens, kSpMaxWidth, up, ntx_total);
  if (rc != DAGPU_OK) return rc;
  if (verify && ntx_total && !account_numbers) return set_err(ctx, DAGPU_ERR_ARG, "null d_account_numbers");
  const size_t at = up.size();
  up.resize(at + kTsMaxChainId, 0);
  if (verify && chain_id_len) memcpy(up.data() + at, chain_id, chain_id_len);
  return DAGPU_OK;
}

namespace {

int ts_host(size_t n, const uint8_t* src, const size_t* src_offs, size_t src_bytes, const uint32_t* ntx,
            const uint64_t* tx_lens, bool verify, const uint8_t* chain_id, size_t chain_id_len,
            const uint64_t* account_numbers, const uint8_t* pubkeys, uint32_t* tx_status, uint32_t* block_status,
            uint8_t* signers) {
  if (n == 0) return DAGPU_OK;
  std::vector<uint8_t> up;
  uint64_t ntx_total = 0;
  const int rc = ts_request(nullptr, n, src, src_offs, src_bytes, ntx, tx_lens, verify, chain_id, chain_id_len,
                            account_numbers, tx_status, block_status, signers, up, ntx_total);
  if (rc != DAGPU_OK) return rc;
  try {
    const TsCarve c = ts_carve(n, ntx_total);
    std::vector<uint64_t> ws((verify ? c.total : c.rec) / 8 + 1);
    uint8_t* w = (uint8_t*)ws.data();
    memset(w, 0xFF, n * 8);
    memcpy(w + c.blk, up.data(), up.size());
    const TsArgs a = ts_args(w, src, n, ntx_total, (uint32_t)chain_id_len, account_numbers, pubkeys, verify, signers,
                             tx_status, block_status);
    ts_run_host(a);
  } catch (const std::bad_alloc&) {
    return set_err(nullptr, DAGPU_ERR_ARG, "out of host memory");
  }
  return DAGPU_OK;
}

}  // namespace
}  // namespace dagpu

extern "C" {

size_t dagpu_tx_sig_verify_workspace_size(size_t n, size_t ntx_total) {
  return (size_t)dagpu::ts_carve(n, ntx_total).total;
}

int dagpu_secp256k1_verify_host(size_t n, const uint8_t* digests, const uint8_t* sigs, const uint8_t* pubkeys,
                                uint32_t* status) {
  using namespace dagpu;
  if (n == 0) return DAGPU_OK;
  if (!digests || !sigs || !pubkeys || !status) return set_err(nullptr, DAGPU_ERR_ARG, "null argument");
  ts_run_raw_host(ts_raw_args(n, digests, sigs, pubkeys, status));
  return DAGPU_OK;
}

int dagpu_secp256k1_g_table(uint8_t* out, int recompute) {
  using namespace dagpu;
  if (!out) return set_err(nullptr, DAGPU_ERR_ARG, "null argument");
  for (uint32_t i = 0; i < 15; i++) {
    if (recompute) {
      secp_g_multiple(i + 1, out + 64 * i);
      continue;
    }
    U256 x, y;
    for (int q = 0; q < 8; q++) {
      x.v[q] = kSecpGHost[i][q];
      y.v[q] = kSecpGHost[i][8 + q];
    }
    u256_to_be(x, out + 64 * i);
    u256_to_be(y, out + 64 * i + 32);
  }
  return DAGPU_OK;
}

int dagpu_tx_signers_host(size_t n, const uint8_t* src, const size_t* src_offs, size_t src_bytes, const uint32_t* ntx,
                          const uint64_t* tx_lens, uint8_t* signers) {
  return dagpu::ts_host(n, src, src_offs, src_bytes, ntx, tx_lens, false, nullptr, 0, nullptr, nullptr, nullptr,
                        nullptr, signers);
}

int dagpu_tx_sig_verify_host(size_t n, const uint8_t* src, const size_t* src_offs, size_t src_bytes,
                             const uint32_t* ntx, const uint64_t* tx_lens, const uint8_t* chain_id,
                             size_t chain_id_len, const uint64_t* account_numbers, const uint8_t* pubkeys,
                             uint32_t* tx_status, uint32_t* block_status, uint8_t* signers) {
  return dagpu::ts_host(n, src, src_offs, src_bytes, ntx, tx_lens, true, chain_id, chain_id_len, account_numbers,
                        pubkeys, tx_status, block_status, signers);
}

}  // extern "C"
