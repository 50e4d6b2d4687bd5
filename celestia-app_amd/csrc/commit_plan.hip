// commit_plan.hip -- the tables of the commitment check laid out on the device
// from the planner's arena and records (dagpu_commit_plan_device,
// dagpu_proposal_check_device), the counted tie of the expected table, and the
// verdict of dagpu_proposal_verdict_device.  The arithmetic is commit_plan.hpp,
// shared with the host executors (commit_plan_host.cpp).
//
//   cp_reduce   one workgroup per block: its blobs' share, subtree and work
//               counts, lanes striding over the plan's blob table.
//   cp_scan     one workgroup: exclusive sums over the n block totals, the
//               counts record, blob_base[n + 1] and the two closing prefix words.
//   cp_fill     one workgroup per block: a scan of its own blobs in LDS, 256 at
//               a time from the block's bases; blob, share_pre and sub_pre by
//               one lane per blob, then the subtree records and the work list
//               by lanes striding over the chunk's subtrees (a binary search in
//               the chunk's prefix sums in LDS finds a subtree's blob).
//   bt_tie_counted  bt_tie over the rows up to blob_base[n], read on the device.
//   pv_fold     one lane per row with a commit status: atomic min of its key
//               into its block's word.
//   pv_finish   one lane per block: the verdict record.
// Hand-offs between kernels go by stream order.  Reads of the arena stay inside
// the plan a record names (cp_block_blobs bounds the record and the header
// against plan_bytes and the arena's capacity); stores stay inside the
// capacities of cp_cap_items / cp_cap_table_words because a block's sums are
// bounded by k * k (cp_block_sums).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "commit_plan_launch.hpp"

namespace dagpu {

namespace {

constexpr uint32_t kCpLanes = 256, kCpWaves = kCpLanes / 64;

// inclusive sums of V values over the 256 lanes; tot[] = the sums over all lanes
template <int V>
__device__ __forceinline__ void cp_scan256(uint32_t (&x)[V], uint32_t (*wave)[kCpWaves], uint32_t (&tot)[V]) {
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
#pragma unroll
  for (int j = 0; j < V; j++) {
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const uint32_t o = __shfl_up(x[j], d);
      if (lane >= d) x[j] += o;
    }
    if (lane == 63) wave[j][w] = x[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < V; j++) {
    uint32_t add = 0, all = 0;
#pragma unroll
    for (uint32_t q = 0; q < kCpWaves; q++) {
      const uint32_t v = wave[j][q];
      add += q < w ? v : 0;
      all += v;
    }
    x[j] += add;
    tot[j] = all;
  }
  __syncthreads();  // wave[] is free again
}

}  // namespace

__global__ __launch_bounds__(kCpLanes) void cp_reduce(CpArgs a) {
  __shared__ uint32_t wave[4][kCpWaves];
  __shared__ uint32_t wmax[kCpWaves], wbad[kCpWaves];
  const uint32_t blk = blockIdx.x, t = threadIdx.x;
  uint32_t nblob;
  const uint32_t* blobs = cp_block_blobs(a.arena, a.arena_cap, a.rec[blk], a.k, &nblob);
  const uint32_t kk = a.k * a.k;
  uint32_t x[4] = {0, 0, 0, 0}, mx = 0, bad = 0;
  for (uint32_t i = t; i < nblob; i += kCpLanes) {
    const CpBlob b = cp_blob(blobs + (uint64_t)i * kSqBlobWords, kk, a.threshold);
    x[1] += b.shares;
    x[2] += b.nsub;
    x[3] += b.nwork;
    mx = b.nsub > mx ? b.nsub : mx;
    bad |= b.bad;
    if (x[1] > kk) {  // past a square already: the lane's sums stay small, the block is out
      bad = 1;
      x[1] = x[2] = x[3] = 0;
    }
  }
  for (uint32_t d = 32; d; d >>= 1) {
    const uint32_t o = __shfl_xor(mx, d);
    mx = o > mx ? o : mx;
  }
  const bool any_bad = __any(bad);
  if ((t & 63) == 0) {
    wmax[t >> 6] = mx;
    wbad[t >> 6] = any_bad;
  }
  uint32_t tot[4];
  cp_scan256<4>(x, wave, tot);
  if (t == 0) {
    uint32_t m = 0, bd = 0;
    for (uint32_t q = 0; q < kCpWaves; q++) {
      m = wmax[q] > m ? wmax[q] : m;
      bd |= wbad[q];
    }
    a.sums[blk] = cp_block_sums(nblob, tot[1], tot[2], tot[3], m, bd != 0, kk);
  }
}

__global__ __launch_bounds__(kCpLanes) void cp_scan(CpArgs a) {
  __shared__ uint32_t wave[4][kCpWaves];
  __shared__ uint32_t wmax[kCpWaves];
  const uint32_t t = threadIdx.x;
  uint32_t carry[4] = {0, 0, 0, 0}, mx = 0;
  for (uint32_t c = 0; c < a.n; c += kCpLanes) {
    const uint32_t i = c + t;
    CpSums s = cp_sums_zero();
    if (i < a.n) s = a.sums[i];
    uint32_t x[4] = {s.nblobs, s.nshares, s.nsub, s.nwork}, tot[4];
    cp_scan256<4>(x, wave, tot);
    if (i < a.n) {
      CpSums b = cp_sums_zero();
      b.nblobs = carry[0] + x[0] - s.nblobs;
      b.nshares = carry[1] + x[1] - s.nshares;
      b.nsub = carry[2] + x[2] - s.nsub;
      b.nwork = carry[3] + x[3] - s.nwork;
      a.base[i] = b;
      a.blob_base[i] = b.nblobs;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) carry[j] += tot[j];
    mx = s.max_subtrees > mx ? s.max_subtrees : mx;
  }
  for (uint32_t d = 32; d; d >>= 1) {
    const uint32_t o = __shfl_xor(mx, d);
    mx = o > mx ? o : mx;
  }
  if ((t & 63) == 0) wmax[t >> 6] = mx;
  __syncthreads();
  if (t == 0) {
    for (uint32_t q = 0; q < kCpWaves; q++) mx = wmax[q] > mx ? wmax[q] : mx;
    a.counts[0] = carry[0];
    a.counts[1] = carry[1];
    a.counts[2] = carry[2];
    a.counts[3] = carry[3];
    a.counts[4] = mx;
    a.counts[5] = a.counts[6] = a.counts[7] = 0;
    a.blob_base[a.n] = carry[0];
    const CpOffsets o = cp_offsets(carry[0], carry[2], carry[3]);
    a.tables[o.share_pre + carry[0]] = carry[1];
    a.tables[o.sub_pre + carry[0]] = carry[2];
  }
}

__global__ __launch_bounds__(kCpLanes) void cp_fill(CpArgs a) {
  __shared__ uint32_t wave[3][kCpWaves];
  __shared__ uint32_t s_share[kCpLanes], s_sub[kCpLanes], s_work[kCpLanes], s_cnt[kCpLanes];
  __shared__ uint8_t s_lw[kCpLanes];
  const uint32_t blk = blockIdx.x, t = threadIdx.x;
  const CpSums mine = a.sums[blk];
  if (mine.nblobs == 0) return;  // uniform over the workgroup
  const CpSums base = a.base[blk];
  const CpOffsets o = cp_offsets(a.counts[0], a.counts[2], a.counts[3]);
  uint32_t nblob;
  const uint32_t* blobs = cp_block_blobs(a.arena, a.arena_cap, a.rec[blk], a.k, &nblob);
  if (nblob != mine.nblobs) return;  // the reduce pass read the same words
  uint32_t carry[3] = {base.nshares, base.nsub, base.nwork};
  for (uint32_t c = 0; c < nblob; c += kCpLanes) {
    const uint32_t i = c + t, in_chunk = nblob - c < kCpLanes ? nblob - c : kCpLanes;
    uint32_t first = 0, count = 0, lw = 0, x[3] = {0, 0, 0}, tot[3];
    if (i < nblob) {
      const uint32_t* rec = blobs + (uint64_t)i * kSqBlobWords;
      first = rec[8];
      count = rec[9];
      lw = cp_log2(cp_subtree_width(count, a.threshold));
      x[0] = count;
      x[1] = cp_subtree_count(count, lw);
      x[2] = cp_work_count(count, lw);
    }
    const uint32_t own[3] = {x[0], x[1], x[2]};
    cp_scan256<3>(x, wave, tot);
    const uint32_t share0 = carry[0] + x[0] - own[0], sub0 = carry[1] + x[1] - own[1],
                   work0 = carry[2] + x[2] - own[2];
    if (i < nblob) {
      const uint64_t g = (uint64_t)base.nblobs + i;
      a.tables[o.blob + 2 * g] = blk;
      a.tables[o.blob + 2 * g + 1] = first;
      a.tables[o.share_pre + g] = share0;
      a.tables[o.sub_pre + g] = sub0;
    }
    s_share[t] = share0;
    s_sub[t] = sub0;
    s_work[t] = work0;
    s_cnt[t] = count;
    s_lw[t] = (uint8_t)lw;
    __syncthreads();
    // the chunk's subtrees [carry[1], carry[1] + tot[1]): every blob has at least
    // one, so s_sub ascends strictly over the chunk's blobs
    for (uint32_t s = t; s < tot[1]; s += kCpLanes) {
      const uint32_t S = carry[1] + s;
      uint32_t lo = 0, hi = in_chunk;  // the last blob with s_sub <= S
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s_sub[mid] <= S) lo = mid;
        else hi = mid;
      }
      cp_put_subtree(a.tables, o, base.nblobs + c + lo, s_cnt[lo], s_lw[lo], s_share[lo], s_sub[lo], s_work[lo],
                     S - s_sub[lo]);
    }
#pragma unroll
    for (int j = 0; j < 3; j++) carry[j] += tot[j];
    __syncthreads();  // the LDS tables are free again
  }
}

__global__ __launch_bounds__(256) void bt_tie_counted(BtArgs a, uint32_t* owner) {
  const uint64_t rows = a.blob_base[a.n];
  for (uint64_t row = blockIdx.x * 256ull + threadIdx.x; row < rows; row += gridDim.x * 256ull)
    bt_tie_row(a, row, owner);
}

__global__ __launch_bounds__(256) void pv_fold(PvArgs a) {
  const uint64_t rows = a.blob_base[a.n];
  for (uint64_t row = blockIdx.x * 256ull + threadIdx.x; row < rows; row += gridDim.x * 256ull) {
    uint32_t blk;
    uint64_t key;
    if (pv_row_key(a, row, &blk, &key)) atomicMin(&a.key[blk], (unsigned long long)key);
  }
}

__global__ __launch_bounds__(256) void pv_finish(PvArgs a) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.n) pv_finish_block(a, i);
}

hipError_t launch_commit_plan(const CpArgs& a, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(cp_reduce, dim3(a.n), dim3(kCpLanes), 0, s, a);
  hipLaunchKernelGGL(cp_scan, dim3(1), dim3(kCpLanes), 0, s, a);
  hipLaunchKernelGGL(cp_fill, dim3(a.n), dim3(kCpLanes), 0, s, a);
  return hipGetLastError();
}

static unsigned row_grid(uint64_t capacity, uint32_t grid_cap) {
  const uint64_t g = (capacity + 255) / 256;
  return (unsigned)(g < grid_cap ? (g ? g : 1) : grid_cap);
}

hipError_t launch_bt_tie_counted(const BtArgs& a, uint32_t* owner, uint64_t capacity, uint32_t grid_cap,
                                 hipStream_t s) {
  if (a.n == 0 || capacity == 0) return hipSuccess;
  hipLaunchKernelGGL(bt_tie_counted, dim3(row_grid(capacity, grid_cap)), dim3(256), 0, s, a, owner);
  return hipGetLastError();
}

hipError_t launch_verdict(const PvArgs& a, uint64_t capacity, uint32_t grid_cap, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  if (capacity) hipLaunchKernelGGL(pv_fold, dim3(row_grid(capacity, grid_cap)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(pv_finish, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dagpu
