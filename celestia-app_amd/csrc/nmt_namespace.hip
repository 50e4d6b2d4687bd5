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
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "forest.hpp"
#include "nmt_node.hpp"
#include "ns_find.hpp"

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

}  // namespace

__global__ __launch_bounds__(256) void ns_find_kernel(NsFindArgs a) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.n_q * a.w) return;
  const long q = t / a.w;
  const long row = t - q * a.w;
  const long w = a.w, ww = w * w;
  const NsKey nid = ns_key_load(a.queries + q * 32);
  // top level of the row store: lvl(log2 w) = 2 w^2 - 2 w (nmt_prove.hip)
  const uint8_t* root = a.row_nodes + (2 * ww - 2 * w + row) * kRecNmt;
  const NsKey rmin = ns_key_load(root), rmax = ns_key_load(root + 32);
  const uint8_t* leaves = a.row_nodes + row * w * kRecNmt;
  uint32_t s, e;
  const int kind = ns_find(nid, rmin, rmax, (uint32_t)w,
                           [&](uint32_t i) { return ns_key_load(leaves + (long)i * kRecNmt); }, &s, &e);
  int32_t* o = a.ranges + t * kNsRangeWords;
  o[0] = kind;
  o[1] = (int32_t)s;
  o[2] = (int32_t)e;
}

__global__ __launch_bounds__(256) void ns_leaf_nodes_kernel(const uint8_t* row_nodes, const int64_t* rec_index, long n,
                                                            uint8_t* out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint8_t* rec = row_nodes + rec_index[i] * kRecNmt;
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

hipError_t launch_ns_leaf_nodes(const uint8_t* row_nodes, const int64_t* rec_index, long n, uint8_t* out,
                                hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(ns_leaf_nodes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, row_nodes, rec_index,
                     n, out);
  return hipGetLastError();
}

}  // namespace dagpu
