// square_write.hip -- the byte-moving pass of square.Construct on the device
// (dagpu_square_write_device, include/dagpu.h): n planned squares of one width
// assembled in HBM from the blocks' raw txs.
//
//   square_write  one wave per 512-B share, 4 shares per block.  The wave's
//                 share index is wave-uniform, so the share's make-up
//                 (sq_share_desc: two or three binary searches over the plan's
//                 tables, which stay in L2) is computed once per wave; lane l
//                 then produces bytes [8 l, 8 l + 8) (sq_share_word: an aligned
//                 8-B load or two with a funnel shift where the 8 bytes lie in
//                 one source segment, a byte loop at a seam) and the wave writes
//                 the share with one coalesced 8-B store per lane.
// The arithmetic is square_write.hpp, shared with the host executor.  The
// kernel trusts its plans: the entry point runs dagpu_square_plan_check on
// every one first, which bounds every table index, literal and txs offset;
// aligned loads round an address down or up by at most 7 bytes inside a word
// that holds a wanted byte.  Stores: share s of square i at
// i * square_stride + (s / k) * row_pitch + (s % k) * 512, s < k * k, i < n.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "runtime.hpp"
#include "square_write.hpp"

namespace dagpu {

namespace {

struct SqBlockRec {
  uint64_t plan_off;  // of the block's plan inside the workspace
  uint64_t src_off;   // of the block's packed txs inside d_src
};

constexpr size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

__global__ __launch_bounds__(256) void square_write_kernel(const uint8_t* __restrict__ ws,
                                                           const uint8_t* __restrict__ src, uint8_t* __restrict__ ods,
                                                           uint32_t log2k, uint64_t shares, uint64_t square_stride,
                                                           uint64_t row_pitch) {
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t g = (uint64_t)blockIdx.x * 4 + wave;
  if (g >= shares) return;
  const uint64_t blk = g >> (2 * log2k);
  const uint32_t s = (uint32_t)(g - (blk << (2 * log2k)));
  const SqBlockRec rec = ((const SqBlockRec*)ws)[blk];
  const uint8_t* plan = ws + rec.plan_off;
  const SqShareDesc d = sq_share_desc(plan, s);
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t w = sq_share_word(d, plan + ((const SqHdr*)plan)->lit_off, src + rec.src_off, lane);
  const uint32_t row = s >> log2k, col = s - (row << log2k);
  uint8_t* o = ods + blk * square_stride + row * row_pitch + (uint64_t)col * kSqShare;
  ((uint64_t*)o)[lane] = w;
}

}  // namespace dagpu

extern "C" {

size_t dagpu_square_write_workspace_size(size_t n, size_t plan_bytes_total) {
  // block records, then every plan at a 16-B aligned offset
  return dagpu::up16(n * sizeof(dagpu::SqBlockRec)) + plan_bytes_total + 16 * n;
}

int dagpu_square_write_device(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* const* plans,
                              const size_t* plan_bytes, const uint8_t* d_src, const size_t* src_offs,
                              size_t src_bytes, uint8_t* d_ods, size_t square_stride, size_t row_pitch,
                              void* d_workspace, void* stream) {
  using namespace dagpu;
  if (!ctx) return DAGPU_ERR_ARG;
  if (n == 0) return DAGPU_OK;
  if (!is_pow2(k) || k > kSqMaxWidth) return set_err(ctx, DAGPU_ERR_ARG, "square width must be a power of two <= 1024");
  if (!plans || !plan_bytes || !src_offs || !d_ods) return set_err(ctx, DAGPU_ERR_ARG, "null argument");
  if (((uintptr_t)d_ods | square_stride | row_pitch | (uintptr_t)d_workspace) & 15)
    return set_err(ctx, DAGPU_ERR_ARG, "d_ods, square_stride, row_pitch and d_workspace must be multiples of 16");
  if (row_pitch < (size_t)k * kSS || (n > 1 && square_stride < (size_t)(k - 1) * row_pitch + (size_t)k * kSS))
    return set_err(ctx, DAGPU_ERR_ARG, "row_pitch below k * 512 or square_stride below one square");
  const uint64_t shares = (uint64_t)n * k * k;
  if (shares > ((uint64_t)1 << 32)) return set_err(ctx, DAGPU_ERR_ARG, "more than 2^32 shares in one call");
  if (src_offs[n] > src_bytes) return set_err(ctx, DAGPU_ERR_ARG, "src_offs end past src_bytes");
  std::vector<SqBlockRec> recs(n);
  size_t at = up16(n * sizeof(SqBlockRec));
  for (size_t i = 0; i < n; i++) {
    if (src_offs[i] > src_offs[i + 1]) return set_err(ctx, DAGPU_ERR_ARG, "src_offs must ascend");
    const size_t len = src_offs[i + 1] - src_offs[i];
    if (len && !d_src) return set_err(ctx, DAGPU_ERR_ARG, "null d_src");
    if (dagpu_square_plan_check(plans[i], plan_bytes[i], len) != DAGPU_OK)
      return set_err(ctx, DAGPU_ERR_ARG, "block " + std::to_string(i) + ": " + thread_err().msg);
    const uint32_t pk = ((const SqHdr*)plans[i])->k;
    if (pk != k)
      return set_err(ctx, DAGPU_ERR_ARG, "block " + std::to_string(i) + " has square width " + std::to_string(pk) +
                                             ", the call writes squares of width " + std::to_string(k));
    recs[i] = {at, src_offs[i]};
    at = up16(at + plan_bytes[i]);
  }
  hipStream_t s = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)d_workspace;
  void* own = nullptr;
  if (!ws) {
    HIP_TRY(ctx, hipMalloc(&own, at));
    ws = (uint8_t*)own;
  }
  hipEvent_t up = ev_take(ctx);
  auto run = [&]() -> int {
    if (!up) return set_err(ctx, DAGPU_ERR_DEVICE, "no event for the plan upload");
    HIP_TRY(ctx, hipMemcpyAsync(ws, recs.data(), n * sizeof(SqBlockRec), hipMemcpyHostToDevice, s));
    for (size_t i = 0; i < n; i++)
      HIP_TRY(ctx, hipMemcpyAsync(ws + recs[i].plan_off, plans[i], plan_bytes[i], hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipEventRecord(up, s));
    uint32_t log2k = 0;
    while ((1u << log2k) < k) log2k++;
    hipLaunchKernelGGL(square_write_kernel, dim3((unsigned)((shares + 3) / 4)), dim3(256), 0, s, ws, d_src, d_ods,
                       log2k, shares, (uint64_t)square_stride, (uint64_t)row_pitch);
    HIP_TRY(ctx, hipGetLastError());
    // the plans and recs are the caller's and this frame's: wait until the
    // upload (not the kernel) has passed
    HIP_TRY(ctx, hipEventSynchronize(up));
    return DAGPU_OK;
  };
  int rc = run();
  if (own) {
    // the kernel reads the library's own workspace: wait for it, then free
    const hipError_t e = hipStreamSynchronize(s);
    if (rc == DAGPU_OK && e != hipSuccess) rc = hip_fail(ctx, e, "hipStreamSynchronize");
    (void)hipFree(own);
  } else if (rc != DAGPU_OK) {
    (void)hipStreamSynchronize(s);  // an upload may still read the caller's plans
  }
  if (up) ev_give(ctx, up);
  return rc;
}

}  // extern "C"
