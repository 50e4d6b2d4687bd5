// ns_find.hpp -- the namespace search of nmt ProveNamespace on one full row
// tree (dagpu_nmt_namespace_ranges_device, nmt_namespace.hip): classify a
// namespace against the tree's root, then find its leaves by binary search.
// Plain arithmetic only (no HIP include), so that tests/host/ns_find_check.cpp
// can compile it without a GPU; every function is marked for both sides when
// hipcc compiles it.
//
// ProveNamespace(tree, nid), root R, leaves sorted by namespace (rules of
// include/dagpu.h, recalled from nmt v0.20.0, IgnoreMaxNamespace):
//   nid < R.min or R.max < nid   outside: the empty proof, start = end = 0
//   leaves with ns == nid exist  present: they are contiguous, [s, e)
//   otherwise                    absent:  s = first leaf with ns > nid, [s, s + 1)
// R.max is the stored one: with IgnoreMaxNamespace a Q0 row's root ignores
// its parity leaves, so the parity namespace is outside rows < k.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DAGPU_NS_HD __host__ __device__
#else
#define DAGPU_NS_HD
#endif

namespace dagpu {

enum NsKind { kNsOutside = 0, kNsPresent = 1, kNsAbsent = 2 };

constexpr int kNsRangeWords = 3;  // int32 per (query, row): kind, start, end

// A 29-B namespace as four big-endian words (bytes 29..31 zero): bytewise
// order is word order.
struct NsKey {
  uint64_t w[4];
};

DAGPU_NS_HD inline bool ns_key_less(const NsKey& a, const NsKey& b) {
  for (int i = 0; i < 4; i++)
    if (a.w[i] != b.w[i]) return a.w[i] < b.w[i];
  return false;
}

// key of 29 bytes at any alignment
DAGPU_NS_HD inline NsKey ns_key_bytes(const uint8_t* p) {
  NsKey k;
  for (int i = 0; i < 4; i++) {
    uint64_t v = 0;
    for (int b = 0; b < 8; b++) v = (v << 8) | (8 * i + b < 29 ? p[8 * i + b] : 0u);
    k.w[i] = v;
  }
  return k;
}

// Classify nid against (rmin, rmax) and search the n leaves; leaf(i) gives the
// key of leaf i and is only called with 0 <= i < n.  start / end are 0 when
// outside; always 0 <= start <= end <= n.
template <class Leaf>
DAGPU_NS_HD inline int ns_find(const NsKey& nid, const NsKey& rmin, const NsKey& rmax, uint32_t n, const Leaf& leaf,
                               uint32_t* start, uint32_t* end) {
  *start = *end = 0;
  if (ns_key_less(nid, rmin) || ns_key_less(rmax, nid)) return kNsOutside;
  uint32_t lo = 0, hi = n;  // lower bound: first leaf with ns >= nid
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (ns_key_less(leaf(mid), nid)) lo = mid + 1; else hi = mid;
  }
  const uint32_t s = lo;
  hi = n;  // upper bound: first leaf with ns > nid
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (ns_key_less(nid, leaf(mid))) hi = mid; else lo = mid + 1;
  }
  if (lo > s) {
    *start = s;
    *end = lo;
    return kNsPresent;
  }
  // nid <= R.max puts a larger leaf in a well-formed tree; a store that has
  // none is answered as outside rather than with an index past the row
  if (s >= n) return kNsOutside;
  *start = s;
  *end = s + 1;
  return kNsAbsent;
}

}  // namespace dagpu
