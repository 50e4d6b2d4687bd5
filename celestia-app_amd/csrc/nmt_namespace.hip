// nmt_namespace.hip -- the namespace search of nmt ProveNamespace over the row
// trees of one resident square (dagpu_nmt_namespace_ranges_device and
// dagpu_nmt_prove_namespace_batch_device, include/dagpu.h).
//
//   ns_find        one lane per (query, row): the row's root record (top level
//                  of the row store) classifies the namespace; only a namespace
//                  inside [R.min, R.max] is searched, by a lower- and an
//                  upper-bound binary search over the 2k level-0 records
//                  (minNs = two 16-B loads per probe, stride 96 B).  The
//                  arithmetic is ns_find.hpp, shared with the host check.
//   ns_leaf_nodes  one lane per absence proof: its level-0 record as a packed
//                  90-B node (the proof's leaf hash).
// Every record index is row * 2k + i with 0 <= row, i < 2k, or the row's root
// record: nothing outside the row store is read.
// The ns_sq_* kernels below run the same search (ns_find_row) across the
// squares of a batch proof store and lay the proofs out on the device.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "forest.hpp"
#include "nmt_node.hpp"
#include "ns_find.hpp"
#include "ns_squares_layout.hpp"

namespace dagpu {

namespace {

// the 32-B zero padded namespace field at p (16-B aligned) as a key
__device__ __forceinline__ NsKey ns_key_load(const uint8_t* p) {
  const uint4* q = (const uint4*)p;
  const uint4 x0 = q[0], x1 = q[1];
  NsKey k;
  k.w[0] = ((uint64_t)__builtin_bswap32(x0.x) << 32) | __builtin_bswap32(x0.y);
  k.w[1] = ((uint64_t)__builtin_bswap32(x0.z) << 32) | __builtin_bswap32(x0.w);
  k.w[2] = ((uint64_t)__builtin_bswap32(x1.x) << 32) | __builtin_bswap32(x1.y);
  k.w[3] = ((uint64_t)__builtin_bswap32(x1.z) << 32) | (__builtin_bswap32(x1.w) & 0xFF000000u);
  return k;
}

// ns_find of query `query` (32 B, padded) on row tree `row` of the row store
// `row_nodes`: the kind, and [*s, *e) unless it is kNsOutside
__device__ __forceinline__ int ns_find_row(const uint8_t* row_nodes, long w, long row, const uint8_t* query,
                                           uint32_t* s, uint32_t* e) {
  // top level of the row store: lvl(log2 w) = 2 w^2 - 2 w (nmt_prove.hip)
  const uint8_t* root = row_nodes + (2 * w * w - 2 * w + row) * kRecNmt;
  const uint8_t* leaves = row_nodes + row * w * kRecNmt;
  return ns_find(ns_key_load(query), ns_key_load(root), ns_key_load(root + 32), (uint32_t)w,
                 [&](uint32_t i) { return ns_key_load(leaves + (long)i * kRecNmt); }, s, e);
}

}  // namespace

__global__ __launch_bounds__(256) void ns_find_kernel(NsFindArgs a) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.n_q * a.w) return;
  const long q = t / a.w;
  const long row = t - q * a.w;
  uint32_t s, e;
  const int kind = ns_find_row(a.row_nodes, a.w, row, a.queries + q * 32, &s, &e);
  int32_t* o = a.ranges + t * kNsRangeWords;
  o[0] = kind;
  o[1] = (int32_t)s;
  o[2] = (int32_t)e;
}

__global__ __launch_bounds__(256) void ns_leaf_nodes_kernel(const uint8_t* base, const int64_t* rec_index, long n,
                                                            uint8_t* out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint8_t* rec = base + rec_index[i] * kRecNmt;
  uint32_t mn[8], mx[8], dg[8];
  load_digest(rec, mn);
  load_digest(rec + 32, mx);
  load_digest(rec + 64, dg);
  write_root(out + i * kNodeSize, mn, mx, dg);
}

hipError_t launch_ns_find(const NsFindArgs& a, hipStream_t s) {
  const long threads = a.n_q * a.w;
  if (threads <= 0) return hipSuccess;
  hipLaunchKernelGGL(ns_find_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ns_leaf_nodes(const uint8_t* base, const int64_t* rec_index, long n, uint8_t* out, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(ns_leaf_nodes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, base, rec_index, n,
                     out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The search across the squares of a batch proof store
// (dagpu_nmt_prove_namespace_squares_device; arithmetic and workspace in
// ns_squares_layout.hpp).  One lane per (query, square, row), t = (query *
// n_sq + square) * w + row, so ascending t is the order of the proofs.
//   find        ns_find_row on the row slice of the lane's square; the result
//               is one packed word (0 = outside)
//   block_sums  the four quantities of a block's 256 lanes, summed
//   scan        exclusive scan of 4-word sums in place, 256 at a time: first
//               every chunk of 256 block sums by a block of its own (its total
//               goes to the chunk sums), then all chunk sums by one block that
//               loops with a carry (its total is the batch's counts)
//   scatter     each hit's position = block offset + chunk offset + its prefix
//               inside the block; it writes the tables the prove kernels read
//               (two-word requests) and the hit record for the host
//   per         one wave per (query, square): the hits among its w lanes
// The leaf hashes of absence proofs are ns_leaf_nodes_kernel's, with record
// indexes counted from the start of the row region (square * records per
// square + row * w + leaf).
// Kernel boundaries are the only synchronisation between workgroups; positions
// come from the scan alone, so the order is the lane order.  Every index is
// below a count the host sized the tables by (lanes, blocks, chunks) or below
// a total it compared with the capacities before the scatter is launched.
// ---------------------------------------------------------------------------
namespace {

struct NsSum {
  int64_t v[kNsSqSums];
};

// Exclusive prefix of x over the 256 lanes of the block and the block's total.
// sh: 4 waves x 4 sums; the two barriers make it reusable in a loop.  v[0]
// counts proofs, so the other three sums are zero wherever it is: a wave with
// no proof at all (most waves: most lanes are outside) skips its shuffles.
__device__ __forceinline__ NsSum ns_block_scan(const NsSum& x, int64_t (*sh)[kNsSqSums], NsSum* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  NsSum inc = x;
  if (__ballot(x.v[0] != 0)) {  // wave-uniform
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
      for (int j = 0; j < kNsSqSums; j++) {
        const int64_t y = __shfl_up(inc.v[j], d, 64);
        if (lane >= d) inc.v[j] += y;
      }
    }
  }
  __syncthreads();  // the previous round's readers are done with sh
  if (lane == 63) {
#pragma unroll
    for (int j = 0; j < kNsSqSums; j++) sh[wave][j] = inc.v[j];
  }
  __syncthreads();
  NsSum ex;
#pragma unroll
  for (int j = 0; j < kNsSqSums; j++) {
    int64_t before = 0, all = 0;
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const int64_t s = sh[v][j];
      if (v < wave) before += s;
      all += s;
    }
    ex.v[j] = before + inc.v[j] - x.v[j];
    total->v[j] = all;
  }
  return ex;
}

}  // namespace

__global__ __launch_bounds__(256) void ns_sq_find_kernel(NsSqArgs a) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.lanes) return;
  const long w = a.w;
  const long pair = t / w, row = t - pair * w;
  const long q = pair / a.n_sq, sq = pair - q * a.n_sq;
  uint32_t s, e;
  const int kind = ns_find_row(a.store + sq * a.row_bytes, w, row, a.queries + q * 32, &s, &e);
  a.words[t] = ns_sq_pack(kind, s, e);
}

__global__ __launch_bounds__(256) void ns_sq_block_sums_kernel(NsSqArgs a) {
  __shared__ int64_t sh[4][kNsSqSums];
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  NsSum x;
  ns_sq_quantities(t < a.lanes ? a.words[t] : 0u, a.logw, x.v);
  NsSum total;
  (void)ns_block_scan(x, sh, &total);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < kNsSqSums; j++) a.bsum[(long)blockIdx.x * kNsSqSums + j] = total.v[j];
  }
}

// Block b scans entries [b * per_block * 256, ...) of v (n entries of 4 sums),
// 256 per round with a carry that starts at 0, exclusive and in place; its
// total goes to out[b].
__global__ __launch_bounds__(256) void ns_sq_scan_kernel(int64_t* v, long n, long per_block, int64_t* out) {
  __shared__ int64_t sh[4][kNsSqSums];
  NsSum carry{};
  const long base = (long)blockIdx.x * per_block * 256;
  for (long r = 0; r < per_block && base + r * 256 < n; r++) {
    const long i = base + r * 256 + threadIdx.x;
    NsSum x{};
    if (i < n) {
#pragma unroll
      for (int j = 0; j < kNsSqSums; j++) x.v[j] = v[i * kNsSqSums + j];
    }
    NsSum total;
    const NsSum ex = ns_block_scan(x, sh, &total);
#pragma unroll
    for (int j = 0; j < kNsSqSums; j++) {
      if (i < n) v[i * kNsSqSums + j] = carry.v[j] + ex.v[j];
      carry.v[j] += total.v[j];
    }
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < kNsSqSums; j++) out[(long)blockIdx.x * kNsSqSums + j] = carry.v[j];
  }
}

__global__ __launch_bounds__(256) void ns_sq_scatter_kernel(NsSqArgs a) {
  __shared__ int64_t sh[4][kNsSqSums];
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const uint32_t word = t < a.lanes ? a.words[t] : 0u;
  NsSum x;
  ns_sq_quantities(word, a.logw, x.v);
  NsSum total;
  const NsSum ex = ns_block_scan(x, sh, &total);
  if (t == 0) {  // the closing entries of the two offset arrays
    a.node_off[a.totals[0]] = a.totals[2];
    a.leaf_off[a.totals[0]] = a.totals[3];
  }
  if (!x.v[0]) return;
  const int64_t* bs = a.bsum + (long)blockIdx.x * kNsSqSums;
  const int64_t* cs = a.csum + (long)(blockIdx.x >> 8) * kNsSqSums;
  const long i = bs[0] + cs[0] + ex.v[0];
  int kind;
  uint32_t s, e;
  ns_sq_unpack(word, &kind, &s, &e);
  const long w = a.w;
  const long pair = t / w, row = t - pair * w;
  const long sq = pair % a.n_sq;
  a.req[2 * i] = (int64_t)(((uint64_t)row << 16) | ((uint64_t)s << 32) | ((uint64_t)e << 48));  // prove_pack_req, axis 0
  a.req[2 * i + 1] = sq;
  a.node_off[i] = bs[2] + cs[2] + ex.v[2];
  a.leaf_off[i] = bs[3] + cs[3] + ex.v[3];
  if (kind == kNsAbsent) a.abs_rec[bs[1] + cs[1] + ex.v[1]] = sq * (a.row_bytes / kRecNmt) + row * w + s;
  a.hits[kNsHitRecWords * i] = (uint32_t)t;
  a.hits[kNsHitRecWords * i + 1] = word;
}

__global__ __launch_bounds__(256) void ns_sq_per_kernel(NsSqArgs a) {
  const long pair = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= a.pairs) return;
  const uint32_t* words = a.words + pair * a.w;
  int n = 0;
  for (int i = threadIdx.x & 63; i < a.w; i += 64) n += (words[i] & 3u) != 0;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) n += __shfl_down(n, d, 64);
  if ((threadIdx.x & 63) == 0) a.per[pair] = n;
}

hipError_t launch_ns_sq_search(const NsSqArgs& a, hipStream_t s) {
  if (a.lanes <= 0) return hipSuccess;
  hipLaunchKernelGGL(ns_sq_find_kernel, dim3((unsigned)a.blocks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(ns_sq_block_sums_kernel, dim3((unsigned)a.blocks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(ns_sq_scan_kernel, dim3((unsigned)a.chunks), dim3(256), 0, s, a.bsum, a.blocks, 1L, a.csum);
  hipLaunchKernelGGL(ns_sq_scan_kernel, dim3(1), dim3(256), 0, s, a.csum, a.chunks, (a.chunks + 255) / 256, a.totals);
  if (a.per) hipLaunchKernelGGL(ns_sq_per_kernel, dim3((unsigned)((a.pairs + 3) / 4)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ns_sq_scatter(const NsSqArgs& a, hipStream_t s) {
  if (a.lanes <= 0) return hipSuccess;
  hipLaunchKernelGGL(ns_sq_scatter_kernel, dim3((unsigned)a.blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dagpu
