// nmt_prove.hip -- batched nmt range proofs from the exported trees of resident
// squares: the producer side of proof_verify.hip.  nmt ProveRange(start, end)
// on the row tree or the column tree of an EDS is a selection of stored nodes;
// nothing is hashed here.  One set of kernels serves the two exports of one
// square (dagpu_nmt_prove_batch_device, include/dagpu.h) and the squares of a
// batch proof store (dagpu_nmt_prove_squares_device; share_proof_layout.hpp):
// ProveArgs gives every region as a base and a per-square stride, and a
// request is one packed word or that word and its square.
//
// Stores (96-B records minNs[32] | maxNs[32] | digest[32], w = 2k):
//   row store   dagpu_row_nodes_device: level L of every row tree after level
//               L - 1, node (row, L, p) at lvl(L) + row * (w >> L) + p with
//               lvl(L) = sum_{l<L} w * (w >> l) = 2 w^2 - (w^2 >> (L - 1)), lvl(0) = 0
//   col store   dagpu_col_nodes_device: levels 1 .. log2(w) of every column tree,
//               node (col, L, p) at lvl(L) - w^2 + col * (w >> L) + p; the leaf
//               of column c at position p is the row store's record p * w + c
//               (the leaf node of a cell is the same in both of its trees).
//
// Four kernels, all index arithmetic and copies:
//   emit        one lane per output node: its proof by binary search in
//               node_off, (depth, position) by the closed form of
//               prove_layout.hpp, one 96-B record in, one packed 90-B node out
//   namespaces  one lane per proof: minNs of the range's first leaf record
//   shares      32 lanes per proven cell, 16 B each: row ranges are contiguous
//               in the EDS, column ranges strided by one EDS row
//   merkle      the merkle half of a proof to the data root, from the DAH trees
//               of a batch proof store (pkg/proof/proof.go:84-91): the axis
//               root, its leaf hash in the DAH tree and the log2(4k) aunts of
//               leaf axis * 2k + index, leaf to root
// The host (prove_host.cpp) has validated every request; the kernels check nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "forest.hpp"
#include "nmt_node.hpp"
#include "prove_layout.hpp"
#include "share_proof_layout.hpp"

namespace dagpu {

struct ProveReq {
  int axis;
  uint32_t index, start, end;
  long sq;
};

// request i: the four uint16 of prove_pack_req and, where the requests carry
// one (a.req_words == 2, the same for every lane), its square
__device__ __forceinline__ ProveReq prove_req(const ProveArgs& a, long i) {
  const uint64_t v = (uint64_t)a.req[i * a.req_words];
  ProveReq r;
  r.axis = (int)(v & 0xFFFFu);
  r.index = (uint32_t)(v >> 16) & 0xFFFFu;
  r.start = (uint32_t)(v >> 32) & 0xFFFFu;
  r.end = (uint32_t)(v >> 48) & 0xFFFFu;
  r.sq = a.req_words == 2 ? a.req[2 * i + 1] : 0;
  return r;
}

// largest i with off[i] <= gid, for 0 <= gid < off[n] (empty proofs are skipped)
__device__ __forceinline__ long prove_find(const int64_t* off, long n, long gid) {
  long lo = 0, hi = n;  // invariant off[lo] <= gid < off[hi]
  while (hi - lo > 1) {
    const long mid = (lo + hi) >> 1;
    if (off[mid] <= gid) lo = mid; else hi = mid;
  }
  return lo;
}

// the 96-B record of node (axis, index, level L, position p) of r's square
__device__ __forceinline__ const uint8_t* prove_record(const ProveArgs& a, const ProveReq& r, int L, uint32_t p) {
  const long w = a.w, ww = w * w;
  const long lvl = L == 0 ? 0 : 2 * ww - (ww >> (L - 1));
  if (r.axis == 0) return a.row_nodes + r.sq * a.row_bytes + (lvl + (long)r.index * (w >> L) + p) * kRecNmt;
  if (L == 0) return a.row_nodes + r.sq * a.row_bytes + ((long)p * w + r.index) * kRecNmt;
  return a.col_inner + r.sq * a.col_bytes + (lvl - ww + (long)r.index * (w >> L) + p) * kRecNmt;
}

// one 96-B record as a packed 90-B node
__device__ __forceinline__ void prove_copy_node(const uint8_t* rec, uint8_t* out) {
  uint32_t mn[8], mx[8], dg[8];
  load_digest(rec, mn);
  load_digest(rec + 32, mx);
  load_digest(rec + 64, dg);
  write_root(out, mn, mx, dg);
}

__global__ __launch_bounds__(256) void prove_emit_kernel(ProveArgs a) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.n_nodes) return;
  const long i = prove_find(a.node_off, a.n, t);
  const ProveReq r = prove_req(a, i);
  int depth;
  uint32_t pos;
  prove_node_at(a.logw, r.start, r.end, (int)(t - a.node_off[i]), &depth, &pos);
  prove_copy_node(prove_record(a, r, a.logw - depth, pos), a.nodes_out + t * kNodeSize);
}

__global__ __launch_bounds__(256) void prove_ns_kernel(ProveArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const ProveReq r = prove_req(a, i);
  uint32_t mn[8];
  load_digest(prove_record(a, r, 0, r.start), mn);
  uint8_t* o = a.ns_out + i * kNsSize;
#pragma unroll
  for (int b = 0; b < kNsSize; b++) o[b] = (uint8_t)(mn[b >> 2] >> (8 * (b & 3)));
}

__global__ __launch_bounds__(256) void prove_shares_kernel(ProveArgs a) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const long cell = t >> 5;  // 32 lanes of 16 B per 512-B cell
  if (cell >= a.n_leaves) return;
  const int q = (int)(t & 31);
  const long i = prove_find(a.leaf_off, a.n, cell);
  const ProveReq r = prove_req(a, i);
  const long j = (long)r.start + (cell - a.leaf_off[i]);  // leaf of the tree
  const long src = r.axis == 0 ? (long)r.index * a.w + j : j * a.w + r.index;
  const uint8_t* eds = a.eds + r.sq * a.square_stride;
  ((uint4*)(a.shares_out + cell * kShareSize))[q] = ((const uint4*)(eds + src * kShareSize))[q];
}

// 2 (log2(4k) + 1) + 1 lanes per proof: two 16-B lanes for the leaf hash and for
// each aunt, one lane for the packed 90-B axis root
__global__ __launch_bounds__(256) void prove_sq_merkle_kernel(ProveArgs a) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const int la = a.logw + 1;  // aunts per proof
  const int per = 2 * (la + 1) + 1;
  const long i = t / per;
  if (i >= a.n) return;
  const int q = (int)(t - i * per);
  const ProveReq r = prove_req(a, i);
  if (q == per - 1) {
    if (a.axis_roots_out) prove_copy_node(prove_record(a, r, a.logw, 0), a.axis_roots_out + i * kNodeSize);
    return;
  }
  const int item = q >> 1, half = q & 1;  // item 0: the leaf hash; item L + 1: the aunt at level L
  const long leaves = 2L * a.w, leaf = (long)r.axis * a.w + r.index;
  const uint4* dah = (const uint4*)(a.dah + r.sq * a.dah_bytes);
  if (item == 0) {
    if (a.leaf_hash_out) ((uint4*)a.leaf_hash_out)[2 * i + half] = dah[2 * leaf + half];
  } else if (a.aunts_out) {
    ((uint4*)a.aunts_out)[2 * (i * la + item - 1) + half] = dah[2 * dah_aunt_at(leaves, leaf, item - 1) + half];
  }
}

hipError_t launch_prove_emit(const ProveArgs& a, hipStream_t s) {
  if (a.n_nodes <= 0) return hipSuccess;
  hipLaunchKernelGGL(prove_emit_kernel, dim3((unsigned)((a.n_nodes + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_prove_namespaces(const ProveArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(prove_ns_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_prove_shares(const ProveArgs& a, hipStream_t s) {
  if (a.n_leaves <= 0) return hipSuccess;
  const long threads = a.n_leaves * 32;
  hipLaunchKernelGGL(prove_shares_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_prove_sq_merkle(const ProveArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  const long threads = a.n * (2 * (a.logw + 2) + 1);
  hipLaunchKernelGGL(prove_sq_merkle_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dagpu
