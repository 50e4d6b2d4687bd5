// tx_sig.hip -- tx signatures over the txs of n blocks resident in HBM
// (dagpu_tx_sig_verify_device, dagpu_tx_signers_device) and the generic batch
// verification (dagpu_secp256k1_verify_device), include/dagpu.h.
//
//   ts_prepare  one lane per tx of the whole batch: ts_walk_tx walks the tx
//               where it lies, stores the signer record and the word the walk
//               alone decides, and for a tx that goes on streams its SignDoc
//               into SHA-256 (ts_sign_doc_hash) and stores the 136-byte
//               record z | r | s | key | pad.  The 16-word block of the hash lies in
//               LDS, [word][lane], so the byte position may index it; a full
//               block goes through sha256.hpp's compression.  Any tx length:
//               lanes diverge on a long tx.
//   ts_verify   one lane per tx (one whose word is already final leaves at
//               once) or per item of the raw call: secp_verify's curve
//               arithmetic, the final word, and for a tx the fold into its
//               block: a rejecting word into lowest (tx index << 32 | word,
//               one 64-bit atomic min), a not-judged one into a counter.
//   ts_finish   one lane per block: the four words of d_block_status.
// The arithmetic is tx_sig.hpp and secp256k1.hpp, shared with the host
// executors (tx_sig_host.cpp).  Reads of src stay inside the tx a lane walks
// (sp_next_field checks every length against the end first); stores go to the
// lane's own tx, item or block.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "runtime.hpp"
#include "sha256.hpp"
#include "tx_sig.hpp"

namespace dagpu {

// ts_sign_doc_hash's sink on the device
struct TsDevSha {
  uint32_t st[8];
  uint32_t* w;  // this lane's column of the block in LDS, 256 words apart
  uint32_t cur, pos;
  __device__ __forceinline__ void put(uint8_t b) {
    cur = cur << 8 | b;
    pos++;
    if ((pos & 3) == 0) {
      w[(((pos >> 2) - 1) & 15) * 256] = cur;
      if ((pos & 63) == 0) {
        uint32_t m[16];
#pragma unroll
        for (int i = 0; i < 16; i++) m[i] = w[i * 256];
        sha256_compress(st, m);
      }
    }
  }
  __device__ __forceinline__ void finish(uint8_t* out) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
      out[4 * i] = (uint8_t)(st[i] >> 24);
      out[4 * i + 1] = (uint8_t)(st[i] >> 16);
      out[4 * i + 2] = (uint8_t)(st[i] >> 8);
      out[4 * i + 3] = (uint8_t)st[i];
    }
  }
};

__global__ __launch_bounds__(256) void ts_prepare(TsArgs a) {
  __shared__ uint32_t block[16 * 256];
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.ntx_total) return;
  TsDevSha sink;
  sha256_init(sink.st);
  sink.w = block + threadIdx.x;
  sink.cur = sink.pos = 0;
  ts_prepare_tx(a, g, sink);
}

__global__ __launch_bounds__(256) void ts_verify(TsVerifyArgs a) {
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.count) return;
  uint32_t blk;
  bool not_judged;
  const uint64_t key = ts_verify_item(a, g, blk, not_judged);
  if (key != ~(uint64_t)0) atomicMin(&a.lowest[blk], (unsigned long long)key);
  if (not_judged) atomicAdd(&a.not_judged[blk], 1u);
}

__global__ __launch_bounds__(256) void ts_finish(TsArgs a) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.n) ts_finish_block(a, i);
}

namespace {

int ts_device(dagpu_ctx* ctx, size_t n, const uint8_t* d_src, const size_t* src_offs, size_t src_bytes,
              const uint32_t* ntx, const uint64_t* tx_lens, bool verify, const uint8_t* chain_id, size_t chain_id_len,
              const uint64_t* d_account_numbers, const uint8_t* d_pubkeys, uint32_t* d_tx_status,
              uint32_t* d_block_status, uint8_t* d_signers, void* d_workspace, void* stream) {
  if (!ctx) return DAGPU_ERR_ARG;
  if (n == 0) return DAGPU_OK;
  if ((uintptr_t)d_workspace & 15) return set_err(ctx, DAGPU_ERR_ARG, "d_workspace must be 16-byte aligned");
  std::vector<uint8_t> up;
  uint64_t ntx_total = 0;
  const int rc0 = ts_request(ctx, n, d_src, src_offs, src_bytes, ntx, tx_lens, verify, chain_id, chain_id_len,
                             d_account_numbers, d_tx_status, d_block_status, d_signers, up, ntx_total);
  if (rc0 != DAGPU_OK) return rc0;
  hipStream_t s = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)d_workspace;
  void* own = nullptr;
  const TsCarve c = ts_carve(n, ntx_total);
  if (!ws) {
    HIP_TRY(ctx, hipMalloc(&own, c.total));
    ws = (uint8_t*)own;
  }
  const TsArgs a = ts_args(ws, d_src, n, ntx_total, (uint32_t)chain_id_len, d_account_numbers, d_pubkeys, verify,
                           d_signers, d_tx_status, d_block_status);
  hipEvent_t done = ev_take(ctx);
  auto run = [&]() -> int {
    if (!done) return set_err(ctx, DAGPU_ERR_DEVICE, "no event for the upload");
    HIP_TRY(ctx, hipMemsetAsync(ws, 0xFF, n * 8, s));
    HIP_TRY(ctx, hipMemsetAsync(ws + c.nj, 0, n * 4, s));
    HIP_TRY(ctx, hipMemcpyAsync(ws + c.blk, up.data(), up.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipEventRecord(done, s));
    if (ntx_total) {
      const dim3 grid((unsigned)((ntx_total + 255) / 256));
      hipLaunchKernelGGL(ts_prepare, grid, dim3(256), 0, s, a);
      HIP_TRY(ctx, hipGetLastError());
      if (verify) {
        hipLaunchKernelGGL(ts_verify, grid, dim3(256), 0, s, ts_verify_args(a));
        HIP_TRY(ctx, hipGetLastError());
      }
    }
    if (verify) {
      hipLaunchKernelGGL(ts_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
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

}  // namespace
}  // namespace dagpu

extern "C" {

int dagpu_secp256k1_verify_device(dagpu_ctx* ctx, size_t n, const uint8_t* d_digests, const uint8_t* d_sigs,
                                  const uint8_t* d_pubkeys, uint32_t* d_status, void* stream) {
  using namespace dagpu;
  if (!ctx) return DAGPU_ERR_ARG;
  if (n == 0) return DAGPU_OK;
  if (!d_digests || !d_sigs || !d_pubkeys || !d_status) return set_err(ctx, DAGPU_ERR_ARG, "null argument");
  if ((uintptr_t)d_status & 3) return set_err(ctx, DAGPU_ERR_ARG, "d_status must be 4-byte aligned");
  if (n >= ((uint64_t)1 << 32)) return set_err(ctx, DAGPU_ERR_UNSUPPORTED, "more than 2^32 signatures in one call");
  hipLaunchKernelGGL(ts_verify, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     ts_raw_args(n, d_digests, d_sigs, d_pubkeys, d_status));
  HIP_TRY(ctx, hipGetLastError());
  return DAGPU_OK;
}

int dagpu_tx_signers_device(dagpu_ctx* ctx, size_t n, const uint8_t* d_src, const size_t* src_offs, size_t src_bytes,
                            const uint32_t* ntx, const uint64_t* tx_lens, uint8_t* d_signers, void* d_workspace,
                            void* stream) {
  return dagpu::ts_device(ctx, n, d_src, src_offs, src_bytes, ntx, tx_lens, false, nullptr, 0, nullptr, nullptr,
                          nullptr, nullptr, d_signers, d_workspace, stream);
}

int dagpu_tx_sig_verify_device(dagpu_ctx* ctx, size_t n, const uint8_t* d_src, const size_t* src_offs,
                               size_t src_bytes, const uint32_t* ntx, const uint64_t* tx_lens, const uint8_t* chain_id,
                               size_t chain_id_len, const uint64_t* d_account_numbers, const uint8_t* d_pubkeys,
                               uint32_t* d_tx_status, uint32_t* d_block_status, uint8_t* d_signers, void* d_workspace,
                               void* stream) {
  return dagpu::ts_device(ctx, n, d_src, src_offs, src_bytes, ntx, tx_lens, true, chain_id, chain_id_len,
                          d_account_numbers, d_pubkeys, d_tx_status, d_block_status, d_signers, d_workspace, stream);
}

}  // extern "C"
