// square_plan.hip -- the layout pass of square.Construct on the device
// (dagpu_square_plan_device, dagpu_square_construct_device, include/dagpu.h):
// the packed txs of n blocks in HBM to n square plans in HBM, and from those
// plans to the squares, with no host step in between.
//
//   sp_classify     one lane per tx of the whole batch: blob.UnmarshalBlobTx in
//                   count mode (sp_classify_tx).
//   sp_plan_blocks  one workgroup of 256 lanes per block: scan of the append
//                   loop, blob records, bitonic sort in LDS, the NextShareIndex
//                   walk on one lane, the PFB stream, the checks and the plan
//                   (sp_plan_block).  The plan's place in the arena comes from
//                   one atomic add per block, so the order of the plans in the
//                   arena is not fixed; each block's record names its plan.
//   square_write_planned  square_write.hip's kernel with the block's plan taken
//                   from the planner's record: a block with a status, or of
//                   another width than the call's, is skipped and its width
//                   reported (kSpWidth).
// The arithmetic is square_plan.hpp, shared with SquareBuilder (square.cpp) and
// with dagpu_square_plan_emulate_host below, which runs the same two functions
// as host loops.  Reads of src stay inside the tx they parse (sp_next_field
// checks every length against the tx's end before it moves), stores inside the
// block's own tables (bounds: sp_carve, sp_plan_bound) and, for the plan, inside
// the arena: a block whose plan would pass arena_cap gets kSpArena and no plan.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "runtime.hpp"
#include "square_plan.hpp"
#include "square_write.hpp"

namespace dagpu {

namespace {

struct SpDeviceLanes {
  template <class F>
  __device__ void each(F&& f) {
    f(threadIdx.x);
    __syncthreads();
  }
  template <class F>
  __device__ void one(F&& f) {
    if (threadIdx.x == 0) f();
    __syncthreads();
  }
  // inclusive sums over the 256 lanes of each row: shuffles inside a wave, the
  // four wave totals through LDS
  __device__ void scan(uint32_t (*v)[kSpLanes], uint32_t (*wave)[kSpLanes / 64]) {
    const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
    uint32_t x[kSpScanVals];
#pragma unroll
    for (uint32_t j = 0; j < kSpScanVals; j++) {
      x[j] = v[j][t];
      for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(x[j], d);
        if (lane >= d) x[j] += o;
      }
      if (lane == 63) wave[j][w] = x[j];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < kSpScanVals; j++) {
      uint32_t add = 0;
      for (uint32_t q = 0; q < kSpLanes / 64; q++) add += q < w ? wave[j][q] : 0;
      v[j][t] = x[j] + add;
    }
    __syncthreads();
  }
  __device__ void lowest(uint32_t* p, uint32_t v) { atomicMin(p, v); }
  __device__ uint64_t clock() { return (uint64_t)wall_clock64(); }  // 100 MHz
  __device__ uint64_t take(unsigned long long* cursor, uint64_t bytes) { return atomicAdd(cursor, (unsigned long long)bytes); }
};

// the host's checks of one call; fills the upload (SpBlockIn[n] | SpTxIn[ntx])
// through sp_tables (square_plan.hpp), which dagpu_blob_tx_validate_* share
int sp_check(dagpu_ctx* ctx, size_t n, const void* src, const size_t* src_offs, size_t src_bytes, const uint32_t* ntx,
             const uint64_t* tx_lens, uint32_t max_square_size, uint32_t threshold, const void* plans,
             const void* records, const void* status, std::vector<uint8_t>& up, uint64_t& ntx_total) {
  if (!is_pow2(max_square_size) || max_square_size > kSpMaxWidth)
    return set_err(ctx, DAGPU_ERR_UNSUPPORTED, "the device planner takes max_square_size a power of two <= 128");
  if (threshold == 0) return set_err(ctx, DAGPU_ERR_ARG, "subtree_root_threshold must be > 0");
  if (!src_offs || !ntx || !plans || !records || !status) return set_err(ctx, DAGPU_ERR_ARG, "null argument");
  if (n >= ((size_t)1 << 24)) return set_err(ctx, DAGPU_ERR_ARG, "more than 2^24 blocks in one call");
  if (((uintptr_t)plans | (uintptr_t)records | (uintptr_t)status) & 15)
    return set_err(ctx, DAGPU_ERR_ARG, "d_plans, d_records and d_status must be 16-byte aligned");
  return sp_tables(ctx, n, src, src_offs, src_bytes, ntx, tx_lens, max_square_size, up, ntx_total);
}

}  // namespace

int sp_tables(dagpu_ctx* ctx, size_t n, const void* src, const size_t* src_offs, size_t src_bytes, const uint32_t* ntx,
              const uint64_t* tx_lens, uint32_t max_square_size, std::vector<uint8_t>& up, uint64_t& ntx_total) {
  if (src_offs[n] > src_bytes) return set_err(ctx, DAGPU_ERR_ARG, "src_offs end past src_bytes");
  ntx_total = 0;
  for (size_t i = 0; i < n; i++) ntx_total += ntx[i];
  if (ntx_total >= ((uint64_t)1 << 32)) return set_err(ctx, DAGPU_ERR_UNSUPPORTED, "more than 2^32 txs in one call");
  if (ntx_total && !tx_lens) return set_err(ctx, DAGPU_ERR_ARG, "tx_lens is required");
  up.resize(n * sizeof(SpBlockIn) + ntx_total * sizeof(SpTxIn));
  SpBlockIn* blk = (SpBlockIn*)up.data();
  SpTxIn* tx = (SpTxIn*)(up.data() + n * sizeof(SpBlockIn));
  uint64_t g = 0;
  for (size_t i = 0; i < n; i++) {
    if (src_offs[i] > src_offs[i + 1]) return set_err(ctx, DAGPU_ERR_ARG, "src_offs must ascend");
    const uint64_t len = src_offs[i + 1] - src_offs[i];
    if (len >= kSqLitFlag)
      return set_err(ctx, DAGPU_ERR_UNSUPPORTED, "a square plan addresses at most 2 GiB of txs");
    if (ntx[i] >= kSpMaxTxs) return set_err(ctx, DAGPU_ERR_UNSUPPORTED, "more than 2^24 txs in one block");
    if (len && !src) return set_err(ctx, DAGPU_ERR_ARG, "null d_src");
    blk[i] = {src_offs[i], (uint64_t)i * max_square_size * max_square_size, (uint32_t)len, (uint32_t)g, ntx[i], 0};
    uint64_t off = 0;
    for (uint32_t j = 0; j < ntx[i]; j++, g++) {
      if (tx_lens[g] > len - off)
        return set_err(ctx, DAGPU_ERR_ARG, "block " + std::to_string(i) + ": tx_lens pass the block's txs");
      tx[g] = {(uint32_t)off, (uint32_t)tx_lens[g], (uint32_t)i, 0};
      off += tx_lens[g];
    }
    if (off != len)
      return set_err(ctx, DAGPU_ERR_ARG, "block " + std::to_string(i) + ": tx_lens do not add up to the block's txs");
  }
  return DAGPU_OK;
}

namespace {

SpArgs sp_args(uint8_t* ws, const uint8_t* src, size_t n, uint64_t ntx_total, uint32_t max_square_size,
               uint32_t threshold, uint8_t* plans, size_t plans_cap, void* records, uint32_t* status) {
  const SpCarve c = sp_carve(n, ntx_total, max_square_size);
  SpArgs a;
  a.src = src;
  a.blk = (const SpBlockIn*)(ws + c.blk);
  a.tx = (const SpTxIn*)(ws + c.tx);
  a.cls = (SpTxCls*)(ws + c.cls);
  a.pos = (SpTxPos*)(ws + c.pos);
  a.sorted = (uint16_t*)(ws + c.sorted);
  a.blobs = (SpBlobRec*)(ws + c.blobs);
  a.arena = plans;
  a.arena_cap = plans_cap;
  a.cursor = (unsigned long long*)ws;
  a.clocks = (unsigned long long*)(ws + c.clocks);
  a.rec = (SpRecord*)records;
  a.status = status;
  a.n = (uint32_t)n;
  a.max_square_size = max_square_size;
  a.threshold = threshold;
  return a;
}

}  // namespace

__global__ __launch_bounds__(256) void sp_classify(SpArgs a, uint64_t ntx_total) {
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g < ntx_total) sp_classify_tx(a, g);
}

__global__ __launch_bounds__(kSpLanes) void sp_plan_blocks(SpArgs a) {
  __shared__ SpShared s;
  SpDeviceLanes x;
  sp_plan_block(x, s, a, blockIdx.x);
}

__global__ __launch_bounds__(256) void square_write_planned(const SpRecord* __restrict__ recs,
                                                            const uint8_t* __restrict__ arena,
                                                            const uint8_t* __restrict__ src, uint8_t* __restrict__ ods,
                                                            uint32_t* __restrict__ status, uint32_t k, uint32_t log2k,
                                                            uint64_t shares, uint64_t square_stride,
                                                            uint64_t row_pitch) {
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t g = (uint64_t)blockIdx.x * 4 + wave;
  if (g >= shares) return;
  const uint64_t blk = g >> (2 * log2k);
  const uint32_t s = (uint32_t)(g - (blk << (2 * log2k)));
  const SpRecord rec = recs[blk];
  const uint32_t lane = threadIdx.x & 63;
  if (rec.status) return;
  if (rec.k != k) {
    if (s == 0 && lane == 0) status[blk] = kSpWidth | (rec.k << 8);
    return;
  }
  const uint8_t* plan = arena + rec.plan_off;
  const SqShareDesc d = sq_share_desc(plan, s);
  const uint64_t w = sq_share_word(d, plan + ((const SqHdr*)plan)->lit_off, src + rec.src_off, lane);
  const uint32_t row = s >> log2k, col = s - (row << log2k);
  uint8_t* o = ods + blk * square_stride + row * row_pitch + (uint64_t)col * kSqShare;
  ((uint64_t*)o)[lane] = w;
}

namespace {

// dagpu_square_plan_device, and with d_ods the writer behind it
int sp_run(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* d_src, const size_t* src_offs, size_t src_bytes,
           const uint32_t* ntx, const uint64_t* tx_lens, uint32_t max_square_size, uint32_t threshold,
           uint8_t* d_plans, size_t plans_cap, void* d_records, uint8_t* d_ods, size_t square_stride,
           size_t row_pitch, uint32_t* d_status, void* d_workspace, void* stream) {
  if (!ctx) return DAGPU_ERR_ARG;
  if (n == 0) return DAGPU_OK;
  if ((uintptr_t)d_workspace & 15) return set_err(ctx, DAGPU_ERR_ARG, "d_workspace must be 16-byte aligned");
  std::vector<uint8_t> up;
  uint64_t ntx_total = 0;
  const int rc0 = sp_check(ctx, n, d_src, src_offs, src_bytes, ntx, tx_lens, max_square_size, threshold, d_plans,
                           d_records, d_status, up, ntx_total);
  if (rc0 != DAGPU_OK) return rc0;
  uint64_t shares = 0;
  uint32_t log2k = 0;
  if (d_ods) {
    if (!is_pow2(k) || k > max_square_size)
      return set_err(ctx, DAGPU_ERR_ARG, "square width must be a power of two <= max_square_size");
    if (((uintptr_t)d_ods | square_stride | row_pitch) & 15)
      return set_err(ctx, DAGPU_ERR_ARG, "d_ods, square_stride and row_pitch must be multiples of 16");
    if (row_pitch < (size_t)k * kSS || (n > 1 && square_stride < (size_t)(k - 1) * row_pitch + (size_t)k * kSS))
      return set_err(ctx, DAGPU_ERR_ARG, "row_pitch below k * 512 or square_stride below one square");
    shares = (uint64_t)n * k * k;
    if (shares > ((uint64_t)1 << 32)) return set_err(ctx, DAGPU_ERR_ARG, "more than 2^32 shares in one call");
    while ((1u << log2k) < k) log2k++;
  }
  hipStream_t s = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)d_workspace;
  void* own = nullptr;
  if (!ws) {
    HIP_TRY(ctx, hipMalloc(&own, sp_carve(n, ntx_total, max_square_size).total));
    ws = (uint8_t*)own;
  }
  const SpArgs a = sp_args(ws, d_src, n, ntx_total, max_square_size, threshold, d_plans, plans_cap, d_records, d_status);
  hipEvent_t done = ev_take(ctx);
  auto run = [&]() -> int {
    if (!done) return set_err(ctx, DAGPU_ERR_DEVICE, "no event for the upload");
    HIP_TRY(ctx, hipMemsetAsync(ws, 0, 16, s));
    HIP_TRY(ctx, hipMemcpyAsync(ws + 16, up.data(), up.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipEventRecord(done, s));
    if (ntx_total) {
      hipLaunchKernelGGL(sp_classify, dim3((unsigned)((ntx_total + 255) / 256)), dim3(256), 0, s, a, ntx_total);
      HIP_TRY(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(sp_plan_blocks, dim3((unsigned)n), dim3(kSpLanes), 0, s, a);
    HIP_TRY(ctx, hipGetLastError());
    if (d_ods) {
      hipLaunchKernelGGL(square_write_planned, dim3((unsigned)((shares + 3) / 4)), dim3(256), 0, s,
                         (const SpRecord*)d_records, (const uint8_t*)d_plans, d_src, d_ods, d_status, k, log2k, shares,
                         (uint64_t)square_stride, (uint64_t)row_pitch);
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

size_t dagpu_square_plan_device_workspace_size(size_t n, size_t ntx_total, uint32_t max_square_size) {
  if (!is_pow2(max_square_size) || max_square_size > dagpu::kSpMaxWidth) return 0;
  return (size_t)dagpu::sp_carve(n, ntx_total, max_square_size).total;
}

size_t dagpu_square_plan_device_arena_size(size_t n, size_t ntx_total, uint32_t max_square_size) {
  if (!is_pow2(max_square_size) || max_square_size > dagpu::kSpMaxWidth) return 0;
  // every block's bound with all txs in it would count them n times; the sum of
  // the per-block bounds is linear in the tx counts
  return (size_t)(dagpu::sp_up16(dagpu::sp_plan_bound(0, max_square_size)) * n +
                  dagpu::sp_up16(dagpu::sp_plan_bound(ntx_total, max_square_size) -
                                 dagpu::sp_plan_bound(0, max_square_size)));
}

int dagpu_square_plan_device(dagpu_ctx* ctx, size_t n, const uint8_t* d_src, const size_t* src_offs, size_t src_bytes,
                             const uint32_t* ntx, const uint64_t* tx_lens, uint32_t max_square_size,
                             uint32_t subtree_root_threshold, uint8_t* d_plans, size_t plans_cap, void* d_records,
                             uint32_t* d_status, void* d_workspace, void* stream) {
  return dagpu::sp_run(ctx, 0, n, d_src, src_offs, src_bytes, ntx, tx_lens, max_square_size, subtree_root_threshold,
                       d_plans, plans_cap, d_records, nullptr, 0, 0, d_status, d_workspace, stream);
}

int dagpu_square_construct_device(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* d_src, const size_t* src_offs,
                                  size_t src_bytes, const uint32_t* ntx, const uint64_t* tx_lens,
                                  uint32_t max_square_size, uint32_t subtree_root_threshold, uint8_t* d_plans,
                                  size_t plans_cap, void* d_records, uint8_t* d_ods, size_t square_stride,
                                  size_t row_pitch, uint32_t* d_status, void* d_workspace, void* stream) {
  if (ctx && !d_ods) return set_err(ctx, DAGPU_ERR_ARG, "null d_ods");
  return dagpu::sp_run(ctx, k, n, d_src, src_offs, src_bytes, ntx, tx_lens, max_square_size, subtree_root_threshold,
                       d_plans, plans_cap, d_records, d_ods, square_stride, row_pitch, d_status, d_workspace, stream);
}

int dagpu_square_plan_emulate_host(size_t n, const uint8_t* src, const size_t* src_offs, size_t src_bytes,
                                   const uint32_t* ntx, const uint64_t* tx_lens, uint32_t max_square_size,
                                   uint32_t subtree_root_threshold, uint8_t* plans, size_t plans_cap, void* records,
                                   uint32_t* status) {
  using namespace dagpu;
  if (n == 0) return DAGPU_OK;
  std::vector<uint8_t> up;
  uint64_t ntx_total = 0;
  const int rc = sp_check(nullptr, n, src, src_offs, src_bytes, ntx, tx_lens, max_square_size, subtree_root_threshold,
                          plans, records, status, up, ntx_total);
  if (rc != DAGPU_OK) return rc;
  try {
    std::vector<uint64_t> ws(sp_carve(n, ntx_total, max_square_size).total / 8 + 1);
    memcpy((uint8_t*)ws.data() + 16, up.data(), up.size());
    const SpArgs a = sp_args((uint8_t*)ws.data(), src, n, ntx_total, max_square_size, subtree_root_threshold, plans,
                             plans_cap, records, status);
    std::vector<SpShared> sh(1);
    sp_emulate(a, ntx_total, sh[0]);
  } catch (const std::bad_alloc&) {
    return set_err(nullptr, DAGPU_ERR_ARG, "out of host memory");
  }
  return DAGPU_OK;
}

}  // extern "C"
