// pipe_carve.hpp -- workspace layout of the sliced dagpu_extend_batch_device.
// Host arithmetic only (no HIP), so that tests/host/pipe_carve_check.cpp can
// compile it without a GPU.
//
// The sliced call hashes slice after slice on the caller's stream.  Every
// slice runs its leaf kernel and tree levels 1..cut over its own squares in
// the slice regions at the front of the workspace (sized for the largest
// slice, reused by every slice); the levels above `cut` run once over all n
// squares after the last slice.  Those launches read
//   * every square's Q0 namespace table (ns_all, 32 B * k^2 * n, filled by
//     each slice's leaf kernel at its own square offset), and
//   * every square's level-`cut` records (rec_c, written by each slice's
//     level-`cut` launch at its own square offset),
// and ping-pong between rec_c and rec_d (level cut+1 records of n squares).
// All of it lies inside dagpu_workspace_size(k, n): with S >= 2 slices the
// slice regions need at most ceil(n / S) / n of what the unsliced call uses.
#pragma once
#include <stddef.h>

namespace dagpu {

inline size_t ws_align256(size_t v) { return (v + 255) & ~(size_t)255; }

inline int nmt_levels(int k) {
  int levels = 0;
  while ((1 << levels) < 2 * k) levels++;
  return levels;
}

// bytes of one square's level-L node records (48 B; 4k trees of 2k >> L nodes)
inline size_t nmt_level_rec_bytes(int k, int L) {
  const size_t w = 2 * (size_t)k;
  return 2 * w * (w >> L) * 48;
}

// One region of a workspace: byte offset from its base and the bytes its
// users address (the next region starts at the following multiple of 256).
struct WsRegion {
  size_t off, bytes;
};

// the unsliced layout: digests | ns_table | rec_a (level 1) | rec_b (level 2)
struct NmtCarve {
  WsRegion digests, ns_table, rec_a, rec_b;
  size_t end;
};

inline NmtCarve nmt_carve(int k, long nsq) {
  NmtCarve c{};
  const size_t w = 2 * (size_t)k;
  size_t p = 0;
  auto take = [&](WsRegion& r, size_t want) {
    r = {p, want};
    p += ws_align256(want);
  };
  take(c.digests, w * w * 32 * nsq);
  take(c.ns_table, (size_t)k * k * 32 * nsq);
  take(c.rec_a, nsq * 2 * w * (w / 2) * 48);
  take(c.rec_b, nsq * 2 * w * (w / 4 > 0 ? w / 4 : 1) * 48);
  c.end = p;
  return c;
}

inline size_t nmt_ws_bytes(int k, long nsq) { return nmt_carve(k, nsq).end; }

// Last tree level that still runs per slice: a level is deferred to the
// batch-wide launch when its launch over a slice of m squares has fewer
// 256-lane workgroups than `fill_blocks` (CUs x resident workgroups per CU of
// the level kernel), i.e. cannot keep every CU at the kernel's occupancy.
// Level 1 reads the slice's leaf digests and always runs per slice.  Returns
// nmt_levels(k) when nothing is deferred.
inline int pipe_cut_level(int k, size_t m, long fill_blocks) {
  const int levels = nmt_levels(k);
  const size_t w = 2 * (size_t)k;
  int cut = 1;
  for (int L = 2; L <= levels; L++) {
    const size_t blocks = (m * 2 * w * (w >> L) + 255) / 256;
    if ((long)blocks < fill_blocks) break;
    cut = L;
  }
  return cut;
}

struct PipeCarve {
  bool defer;  // false: nothing deferred or no room; every slice uses the unsliced layout for its own squares
  int cut;     // levels 1..cut per slice, cut+1..levels once over the batch
  // byte offsets into the workspace and sizes; slice regions hold m squares
  size_t digests, digests_bytes, rec_a, rec_a_bytes, rec_b, rec_b_bytes;
  size_t ns_all, ns_all_bytes, rec_c, rec_c_bytes, rec_d, rec_d_bytes;
  size_t end;
};

// n squares, largest slice m (< n when sliced), levels above `cut` deferred;
// `limit` = dagpu_workspace_size(k, n)
inline PipeCarve pipe_carve(int k, size_t n, size_t m, int cut, size_t limit) {
  PipeCarve c{};
  const int levels = nmt_levels(k);
  const size_t w = 2 * (size_t)k;
  c.cut = cut;
  if (cut < 1 || cut >= levels || m == 0 || m >= n) return c;
  size_t p = 0;
  auto take = [&](size_t& off, size_t& bytes, size_t want) {
    off = p;
    bytes = want;
    p += ws_align256(want);
  };
  take(c.digests, c.digests_bytes, w * w * 32 * m);
  take(c.rec_a, c.rec_a_bytes, m * nmt_level_rec_bytes(k, 1));
  take(c.rec_b, c.rec_b_bytes, m * nmt_level_rec_bytes(k, 2));
  take(c.ns_all, c.ns_all_bytes, (size_t)k * k * 32 * n);
  take(c.rec_c, c.rec_c_bytes, n * nmt_level_rec_bytes(k, cut));
  take(c.rec_d, c.rec_d_bytes, n * nmt_level_rec_bytes(k, cut + 1));
  c.end = p;
  c.defer = p <= limit;
  return c;
}

}  // namespace dagpu
