// blob_commit.hip -- inclusion.CreateCommitment (pkg/inclusion/commitment.go:19-75)
// for every blob of a batch of squares resident in HBM
// (dagpu_blob_commitments_device, include/dagpu.h).  Three launches per call,
// whatever the number of squares, blobs or shares:
//
//   commit_leaf     one lane per blob share over the whole batch.  The lane
//                   finds its blob by binary search in the share prefix sums,
//                   reads its share through the square's stride and pitch and
//                   writes the nmt leaf record 0x00 | share[0:29] | share
//                   (share_leaf_sha256, the Q0 rule of the wrapper) at its own
//                   index: a blob's records are consecutive, so every subtree of
//                   the mountain range is one run of them.
//   commit_subtree  one wave per subtree of 2 .. 1024 leaves.  Level by level,
//                   lanes striding over the nodes, nmt HashNode with
//                   IgnoreMaxNamespace; the levels alternate between the leaf
//                   records and the `inner` array, each subtree inside its own
//                   window of both, with a workgroup barrier between levels.
//                   Level 1 applies nmt's push-order rule to the leaves.
//   commit_root     one wave per blob: RFC-6962 leaf digests of its subtree
//                   roots (0x00 | 90 B), then pairwise levels with the odd node
//                   carried up (merkle.HashFromByteSlices), alternating between
//                   two digest arrays; then the compare and the status words.
//
// The kernels check nothing: commit_layout.hpp bounded every table entry, and
// the entry point the geometry, before anything was enqueued.  Reads of the
// squares: share s of square i at i * square_stride + (s / k) * row_pitch +
// (s % k) * 512 with s < k * k and i < n.  Hand-offs between levels stay inside
// one workgroup (barrier); between kernels the stream orders them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dagpu.h"
#include "forest.hpp"
#include "nmt_node.hpp"
#include "sha256.hpp"

namespace dagpu {

namespace {

__device__ __forceinline__ void ld8(const uint8_t* p, uint32_t (&d)[8]) {
  const uint4* q = (const uint4*)p;
  const uint4 x0 = q[0], x1 = q[1];
  d[0] = x0.x; d[1] = x0.y; d[2] = x0.z; d[3] = x0.w;
  d[4] = x1.x; d[5] = x1.y; d[6] = x1.z; d[7] = x1.w;
}

__device__ __forceinline__ void st8(uint8_t* p, const uint32_t (&d)[8]) {
  uint4* q = (uint4*)p;
  q[0] = make_uint4(d[0], d[1], d[2], d[3]);
  q[1] = make_uint4(d[4], d[5], d[6], d[7]);
}

// SHA-256 of the `len`-byte message in m (little-endian packed, zero past len,
// len + 9 <= 128): two blocks.  out in byte order.
template <int LEN>
__device__ __forceinline__ void sha_two_blocks(uint32_t (&m)[32], uint32_t (&out)[8]) {
  m[LEN >> 2] |= 0x80u << (8 * (LEN & 3));
  uint32_t st[8];
  sha256_init(st);
#pragma unroll
  for (int blk = 0; blk < 2; blk++) {
    uint32_t wv[16];
#pragma unroll
    for (int j = 0; j < 16; j++) wv[j] = bswap32(m[16 * blk + j]);
    if (blk == 1) { wv[14] = 0; wv[15] = (uint32_t)LEN * 8u; }
    sha256_compress(st, wv);
  }
#pragma unroll
  for (int j = 0; j < 8; j++) out[j] = bswap32(st[j]);
}

// merkle leafHash of a 90-B nmt root: SHA256(0x00 | min(29) | max(29) | digest(32))
__device__ __forceinline__ void rfc_leaf_of_root(const uint8_t* rec, uint32_t (&out)[8]) {
  uint32_t mn[8], mx[8], dg[8];
  ld8(rec, mn); ld8(rec + 32, mx); ld8(rec + 64, dg);
  mn[7] &= 0xFFu;
  mx[7] &= 0xFFu;
  uint32_t m[32];
#pragma unroll
  for (int j = 0; j < 32; j++) m[j] = 0;
  put_bytes<1>(m, mn);
  put_bytes<1 + 29>(m, mx);
  put_bytes<1 + 58>(m, dg);
  sha_two_blocks<91>(m, out);
}

// merkle innerHash SHA256(0x01 | l | r)
__device__ __forceinline__ void rfc_inner_hash(const uint32_t (&l)[8], const uint32_t (&r)[8], uint32_t (&out)[8]) {
  uint32_t m[32];
#pragma unroll
  for (int j = 0; j < 32; j++) m[j] = 0;
  m[0] = 0x01u;
  put_bytes<1>(m, l);
  put_bytes<33>(m, r);
  sha_two_blocks<65>(m, out);
}

}  // namespace

// leaf record g of the batch
__device__ __forceinline__ void commit_leaf_body(const CommitArgs& a, uint32_t g) {
  uint32_t lo = 0, hi = a.nblobs;  // share_pre[lo] <= g < share_pre[hi]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a.share_pre[mid] <= g) lo = mid; else hi = mid;
  }
  const uint32_t sq = a.blob[2 * lo], s = a.blob[2 * lo + 1] + (g - a.share_pre[lo]);
  const uint32_t row = s >> a.log2k, col = s - (row << a.log2k);
  const uint8_t* src = a.squares + sq * a.square_stride + row * a.row_pitch + (uint64_t)col * kShareSize;
  uint32_t st[8], ns[8];
  share_leaf_sha256((const uint4*)src, true, st, ns);
  uint4* o = (uint4*)(a.leaves + (uint64_t)g * kRecNmt);
  o[0] = make_uint4(ns[0], ns[1], ns[2], ns[3]);
  o[1] = make_uint4(ns[4], ns[5], ns[6], ns[7]);
  o[2] = o[0];
  o[3] = o[1];
  o[4] = make_uint4(bswap32(st[0]), bswap32(st[1]), bswap32(st[2]), bswap32(st[3]));
  o[5] = make_uint4(bswap32(st[4]), bswap32(st[5]), bswap32(st[6]), bswap32(st[7]));
}

__global__ __launch_bounds__(256) void commit_leaf_kernel(CommitArgs a) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g < a.nshares) commit_leaf_body(a, g);
}

// work item `item` by one wave; ends behind a workgroup barrier
__device__ __forceinline__ void commit_subtree_body(const CommitArgs& a, uint32_t item) {
  const uint32_t* q = a.sub + 3 * a.work[item];
  const uint32_t blob = q[0], first = q[1], size = q[2];
  // level L reads level L - 1: odd levels live in `inner`, even ones (the
  // leaves are level 0) in the leaf records, this subtree's window of each
  uint8_t* even = a.leaves + (uint64_t)first * kRecNmt;
  uint8_t* odd = a.inner + (uint64_t)(first >> 1) * kRecNmt;
  bool bad = false;
  int level = 1;
  for (uint32_t cnt = size; cnt > 1; cnt >>= 1, level++) {
    const uint8_t* in = (level & 1) ? even : odd;
    uint8_t* out = (level & 1) ? odd : even;
    for (uint32_t j = threadIdx.x; j < cnt / 2; j += 64) {
      const uint8_t* lp = in + (uint64_t)(2 * j) * kRecNmt;
      const uint8_t* rp = lp + kRecNmt;
      uint32_t lmn[8], lmx[8], ld[8], rmn[8], rmx[8], rd[8];
      ld8(lp, lmn); ld8(lp + 32, lmx); ld8(lp + 64, ld);
      ld8(rp, rmn); ld8(rp + 32, rmx); ld8(rp + 64, rd);
      if (level == 1) {  // nmt Push: ns(2j) <= ns(2j + 1) <= ns(2j + 2)
        bad |= ns_less(rmn, lmn);
        if (2 * j + 2 < cnt) {
          uint32_t n2[8];
          ld8(rp + kRecNmt, n2);
          bad |= ns_less(n2, rmn);
        }
      }
      auto get = [&](int P, int i) -> uint32_t {
        return P == 0 ? lmn[i] : P == 1 ? lmx[i] : P == 2 ? ld[i] : P == 3 ? rmn[i] : P == 4 ? rmx[i] : rd[i];
      };
      uint32_t st[8];
      sha_node_msg(get, st);
      uint32_t dg[8];
#pragma unroll
      for (int i = 0; i < 8; i++) dg[i] = bswap32(st[i]);
      uint8_t* op = out + (uint64_t)j * kRecNmt;
      st8(op, lmn);
      if (ns_is_parity(rmn)) st8(op + 32, lmx); else st8(op + 32, rmx);  // IgnoreMaxNamespace
      st8(op + 64, dg);
    }
    __syncthreads();
  }
  if (bad) atomicOr(&a.status[blob], DAGPU_COMMIT_PUSH_ORDER);
}

__global__ __launch_bounds__(64) void commit_subtree_kernel(CommitArgs a) { commit_subtree_body(a, blockIdx.x); }

// blob b by one wave
__device__ __forceinline__ void commit_root_body(const CommitArgs& a, uint32_t b) {
  const uint32_t lane = threadIdx.x;
  const uint32_t s0 = a.sub_pre[b], T = a.sub_pre[b + 1] - s0;
  uint8_t* d0 = a.dig0 + (uint64_t)s0 * 32;
  uint8_t* d1 = a.dig1 + (uint64_t)s0 * 32;
  for (uint32_t i = lane; i < T; i += 64) {
    const uint32_t* q = a.sub + 3 * (s0 + i);
    const uint32_t first = q[1], size = q[2];
    // a subtree of 2^L leaves left its root on level L (commit_subtree_kernel)
    const bool in_inner = (31 - __builtin_clz(size)) & 1;
    const uint8_t* rec = in_inner ? a.inner + (uint64_t)(first >> 1) * kRecNmt : a.leaves + (uint64_t)first * kRecNmt;
    uint32_t dg[8];
    rfc_leaf_of_root(rec, dg);
    st8(d0 + (uint64_t)i * 32, dg);
  }
  __syncthreads();
  int lvl = 0;
  for (uint32_t cnt = T; cnt > 1; lvl++) {
    const uint8_t* in = (lvl & 1) ? d1 : d0;
    uint8_t* out = (lvl & 1) ? d0 : d1;
    const uint32_t half = (cnt + 1) / 2;
    for (uint32_t j = lane; j < half; j += 64) {
      uint32_t l[8], o[8];
      ld8(in + (uint64_t)(2 * j) * 32, l);
      if (2 * j + 1 < cnt) {
        uint32_t r[8];
        ld8(in + (uint64_t)(2 * j + 1) * 32, r);
        rfc_inner_hash(l, r, o);
        st8(out + (uint64_t)j * 32, o);
      } else {
        st8(out + (uint64_t)j * 32, l);  // odd node out: carried up unchanged
      }
    }
    __syncthreads();
    cnt = half;
  }
  const uint8_t* fin = (lvl & 1) ? d1 : d0;
  bool differ = false;
  if (lane < 32) {
    const uint8_t v = fin[lane];
    a.commitments[(uint64_t)b * 32 + lane] = v;
    if (a.expected) differ = a.expected[(uint64_t)b * 32 + lane] != v;
  }
  const bool mismatch = __any(differ);
  if (lane == 0) {
    const int st = a.status[b] | (mismatch ? DAGPU_COMMIT_MISMATCH : 0);
    a.status[b] = st;
    if (a.square_status && st) atomicOr(&a.square_status[a.blob[2 * b]], st);
  }
}

__global__ __launch_bounds__(64) void commit_root_kernel(CommitArgs a) { commit_root_body(a, blockIdx.x); }

// ---- the counted forms (dagpu_proposal_check_device) ---------------------------------
// The tables were laid out on the device (commit_plan.hip), so the host knows
// neither the counts nor where each table starts inside the image: every
// workgroup reads the counts record (uniform loads) and strides over the items.
// The launch is sized by the capacity and a cap; a workgroup past the count
// leaves at once.
__device__ __forceinline__ CommitArgs commit_counted_args(const CommitCounted& c) {
  CommitArgs a = c.a;
  a.nblobs = c.counts[0];
  a.nshares = c.counts[1];
  a.nsub = c.counts[2];
  a.nwork = c.counts[3];
  const uint64_t o_share_pre = 2 * (uint64_t)a.nblobs, o_sub_pre = o_share_pre + a.nblobs + 1;
  const uint64_t o_sub = o_sub_pre + a.nblobs + 1;
  a.blob = c.tables;
  a.share_pre = c.tables + o_share_pre;
  a.sub_pre = c.tables + o_sub_pre;
  a.sub = c.tables + o_sub;
  a.work = c.tables + o_sub + 3 * (uint64_t)a.nsub;
  return a;
}

__global__ __launch_bounds__(256) void commit_leaf_counted_kernel(CommitCounted c) {
  const CommitArgs a = commit_counted_args(c);
  for (uint64_t g = blockIdx.x * 256ull + threadIdx.x; g < a.nshares; g += gridDim.x * 256ull)
    commit_leaf_body(a, (uint32_t)g);
}

// the loop bounds are uniform over the workgroup: the barriers inside the bodies are legal
__global__ __launch_bounds__(64) void commit_subtree_counted_kernel(CommitCounted c) {
  const CommitArgs a = commit_counted_args(c);
  for (uint32_t i = blockIdx.x; i < a.nwork; i += gridDim.x) commit_subtree_body(a, i);
}

__global__ __launch_bounds__(64) void commit_root_counted_kernel(CommitCounted c) {
  const CommitArgs a = commit_counted_args(c);
  for (uint32_t b = blockIdx.x; b < a.nblobs; b += gridDim.x) commit_root_body(a, b);
}

hipError_t launch_commit_leaves(const CommitArgs& a, hipStream_t s) {
  if (a.nshares == 0) return hipSuccess;
  hipLaunchKernelGGL(commit_leaf_kernel, dim3((a.nshares + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_commit_subtrees(const CommitArgs& a, hipStream_t s) {
  if (a.nwork == 0) return hipSuccess;
  hipLaunchKernelGGL(commit_subtree_kernel, dim3(a.nwork), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_commit_roots(const CommitArgs& a, hipStream_t s) {
  if (a.nblobs == 0) return hipSuccess;
  hipLaunchKernelGGL(commit_root_kernel, dim3(a.nblobs), dim3(64), 0, s, a);
  return hipGetLastError();
}

static unsigned counted_grid(uint64_t capacity_groups, uint32_t grid_cap) {
  const uint64_t g = capacity_groups < grid_cap ? capacity_groups : grid_cap;
  return (unsigned)(g ? g : 1);
}

hipError_t launch_commit_leaves_counted(const CommitCounted& c, uint64_t capacity, uint32_t grid_cap, hipStream_t s) {
  if (capacity == 0) return hipSuccess;
  hipLaunchKernelGGL(commit_leaf_counted_kernel, dim3(counted_grid((capacity + 255) / 256, grid_cap)), dim3(256), 0, s, c);
  return hipGetLastError();
}

hipError_t launch_commit_subtrees_counted(const CommitCounted& c, uint64_t capacity, uint32_t grid_cap, hipStream_t s) {
  if (capacity == 0) return hipSuccess;
  hipLaunchKernelGGL(commit_subtree_counted_kernel, dim3(counted_grid(capacity, grid_cap)), dim3(64), 0, s, c);
  return hipGetLastError();
}

hipError_t launch_commit_roots_counted(const CommitCounted& c, uint64_t capacity, uint32_t grid_cap, hipStream_t s) {
  if (capacity == 0) return hipSuccess;
  hipLaunchKernelGGL(commit_root_counted_kernel, dim3(counted_grid(capacity, grid_cap)), dim3(64), 0, s, c);
  return hipGetLastError();
}

}  // namespace dagpu
