// nmt_prove.hip -- batched nmt range proofs from the exported trees of one
// resident square (dagpu_nmt_prove_batch_device, include/dagpu.h): the producer
// side of proof_verify.hip.  nmt ProveRange(start, end) on the row tree or the
// column tree of an EDS is a selection of stored nodes; nothing is hashed here.
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
// Three kernels, all index arithmetic and copies:
//   emit        one lane per output node: its proof by binary search in
//               node_off, (depth, position) by the closed form of
//               prove_layout.hpp, one 96-B record in, one packed 90-B node out
//   namespaces  one lane per proof: minNs of the range's first leaf record
//   shares      32 lanes per proven cell, 16 B each: row ranges are contiguous
//               in the EDS, column ranges strided by one EDS row
// The host (trees.cpp) has validated every request; the kernels check nothing.
// The prove_sq_* kernels below serve requests across the squares of a batch
// proof store and add the merkle half to the data root.
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
};

__device__ __forceinline__ ProveReq prove_unpack(uint64_t v) {
  ProveReq r;
  r.axis = (int)(v & 0xFFFFu);
  r.index = (uint32_t)(v >> 16) & 0xFFFFu;
  r.start = (uint32_t)(v >> 32) & 0xFFFFu;
  r.end = (uint32_t)(v >> 48) & 0xFFFFu;
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

// the 96-B record of node (axis, index, level L, position p)
__device__ __forceinline__ const uint8_t* prove_record(const ProveArgs& a, int axis, uint32_t index, int L,
                                                       uint32_t p) {
  const long w = a.w, ww = w * w;
  if (L == 0) return a.row_nodes + (axis == 0 ? (long)index * w + p : (long)p * w + index) * kRecNmt;
  const long lvl = 2 * ww - (ww >> (L - 1));
  const long in_level = (long)index * (w >> L) + p;
  return axis == 0 ? a.row_nodes + (lvl + in_level) * kRecNmt : a.col_inner + (lvl - ww + in_level) * kRecNmt;
}

__device__ __forceinline__ void prove_load8(const uint8_t* p, uint32_t (&d)[8]) {
  const uint4* q = (const uint4*)p;
  const uint4 x0 = q[0], x1 = q[1];
  d[0] = x0.x; d[1] = x0.y; d[2] = x0.z; d[3] = x0.w;
  d[4] = x1.x; d[5] = x1.y; d[6] = x1.z; d[7] = x1.w;
}

__global__ __launch_bounds__(256) void prove_emit_kernel(ProveArgs a) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.n_nodes) return;
  const long i = prove_find(a.node_off, a.n, t);
  const ProveReq r = prove_unpack(a.req[i]);
  int depth;
  uint32_t pos;
  prove_node_at(a.logw, r.start, r.end, (int)(t - a.node_off[i]), &depth, &pos);
  const uint8_t* rec = prove_record(a, r.axis, r.index, a.logw - depth, pos);
  uint32_t mn[8], mx[8], dg[8];
  prove_load8(rec, mn);
  prove_load8(rec + 32, mx);
  prove_load8(rec + 64, dg);
  write_root(a.nodes_out + t * kNodeSize, mn, mx, dg);
}

__global__ __launch_bounds__(256) void prove_ns_kernel(ProveArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const ProveReq r = prove_unpack(a.req[i]);
  uint32_t mn[8];
  prove_load8(prove_record(a, r.axis, r.index, 0, r.start), mn);
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
  const ProveReq r = prove_unpack(a.req[i]);
  const long j = (long)r.start + (cell - a.leaf_off[i]);  // leaf of the tree
  const long src = r.axis == 0 ? (long)r.index * a.w + j : j * a.w + r.index;
  ((uint4*)(a.shares_out + cell * kShareSize))[q] = ((const uint4*)(a.eds + src * kShareSize))[q];
}

// ---------------------------------------------------------------------------
// The same three kernels across the squares of a batch proof store
// (dagpu_nmt_prove_squares_device; layout in share_proof_layout.hpp): request
// i carries its square, whose row and column slices of the store are the two
// stores above, and whose cells lie square_stride bytes after the previous
// square's.  A fourth kernel copies the merkle half of a proof to the data
// root (pkg/proof/proof.go:84-91): the axis root, its leaf hash in the DAH tree
// and the log2(4k) aunts of leaf axis * 2k + index, leaf to root.
// ---------------------------------------------------------------------------
__device__ __forceinline__ ProveArgs prove_sq_view(const ProveSqArgs& a, long sq) {
  ProveArgs v{};
  v.w = a.w;
  v.logw = a.logw;
  v.row_nodes = a.store + sq * a.row_bytes;
  v.col_inner = a.store + a.col_off + sq * a.col_bytes;
  v.eds = a.eds + sq * a.square_stride;
  return v;
}

__global__ __launch_bounds__(256) void prove_sq_emit_kernel(ProveSqArgs a) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.n_nodes) return;
  const long i = prove_find(a.node_off, a.n, t);
  const ProveReq r = prove_unpack((uint64_t)a.req[2 * i]);
  int depth;
  uint32_t pos;
  prove_node_at(a.logw, r.start, r.end, (int)(t - a.node_off[i]), &depth, &pos);
  const uint8_t* rec = prove_record(prove_sq_view(a, a.req[2 * i + 1]), r.axis, r.index, a.logw - depth, pos);
  uint32_t mn[8], mx[8], dg[8];
  prove_load8(rec, mn);
  prove_load8(rec + 32, mx);
  prove_load8(rec + 64, dg);
  write_root(a.nodes_out + t * kNodeSize, mn, mx, dg);
}

__global__ __launch_bounds__(256) void prove_sq_ns_kernel(ProveSqArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const ProveReq r = prove_unpack((uint64_t)a.req[2 * i]);
  uint32_t mn[8];
  prove_load8(prove_record(prove_sq_view(a, a.req[2 * i + 1]), r.axis, r.index, 0, r.start), mn);
  uint8_t* o = a.ns_out + i * kNsSize;
#pragma unroll
  for (int b = 0; b < kNsSize; b++) o[b] = (uint8_t)(mn[b >> 2] >> (8 * (b & 3)));
}

__global__ __launch_bounds__(256) void prove_sq_shares_kernel(ProveSqArgs a) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const long cell = t >> 5;  // 32 lanes of 16 B per 512-B cell
  if (cell >= a.n_leaves) return;
  const int q = (int)(t & 31);
  const long i = prove_find(a.leaf_off, a.n, cell);
  const ProveReq r = prove_unpack((uint64_t)a.req[2 * i]);
  const long j = (long)r.start + (cell - a.leaf_off[i]);  // leaf of the tree
  const long src = r.axis == 0 ? (long)r.index * a.w + j : j * a.w + r.index;
  const uint8_t* eds = a.eds + a.req[2 * i + 1] * a.square_stride;
  ((uint4*)(a.shares_out + cell * kShareSize))[q] = ((const uint4*)(eds + src * kShareSize))[q];
}

// 2 (log2(4k) + 1) + 1 lanes per proof: two 16-B lanes for the leaf hash and for
// each aunt, one lane for the packed 90-B axis root
__global__ __launch_bounds__(256) void prove_sq_merkle_kernel(ProveSqArgs a) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const int la = a.logw + 1;  // aunts per proof
  const int per = 2 * (la + 1) + 1;
  const long i = t / per;
  if (i >= a.n) return;
  const int q = (int)(t - i * per);
  const ProveReq r = prove_unpack((uint64_t)a.req[2 * i]);
  const long sq = a.req[2 * i + 1];
  if (q == per - 1) {
    if (!a.axis_roots_out) return;
    const uint8_t* rec = prove_record(prove_sq_view(a, sq), r.axis, r.index, a.logw, 0);
    uint32_t mn[8], mx[8], dg[8];
    prove_load8(rec, mn);
    prove_load8(rec + 32, mx);
    prove_load8(rec + 64, dg);
    write_root(a.axis_roots_out + i * kNodeSize, mn, mx, dg);
    return;
  }
  const int item = q >> 1, half = q & 1;  // item 0: the leaf hash; item L + 1: the aunt at level L
  const long leaves = 2L * a.w, leaf = (long)r.axis * a.w + r.index;
  const uint4* dah = (const uint4*)(a.store + a.dah_off + sq * a.dah_bytes);
  if (item == 0) {
    if (a.leaf_hash_out) ((uint4*)a.leaf_hash_out)[2 * i + half] = dah[2 * leaf + half];
  } else if (a.aunts_out) {
    ((uint4*)a.aunts_out)[2 * (i * la + item - 1) + half] = dah[2 * dah_aunt_at(leaves, leaf, item - 1) + half];
  }
}

hipError_t launch_prove_sq_emit(const ProveSqArgs& a, hipStream_t s) {
  if (a.n_nodes <= 0) return hipSuccess;
  hipLaunchKernelGGL(prove_sq_emit_kernel, dim3((unsigned)((a.n_nodes + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_prove_sq_namespaces(const ProveSqArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(prove_sq_ns_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_prove_sq_shares(const ProveSqArgs& a, hipStream_t s) {
  if (a.n_leaves <= 0) return hipSuccess;
  const long threads = a.n_leaves * 32;
  hipLaunchKernelGGL(prove_sq_shares_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_prove_sq_merkle(const ProveSqArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  const long threads = a.n * (2 * (a.logw + 2) + 1);
  hipLaunchKernelGGL(prove_sq_merkle_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
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

}  // namespace dagpu
