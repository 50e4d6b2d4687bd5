// repair_layout.hpp -- workspace layout of Repair (repair_host.cpp; the size
// callers allocate is dagpu_repair_workspace_size).  Host arithmetic only (no
// HIP), so that tests/host/repair_layout_check.cpp can compile it without a
// GPU.  One walk over one list of regions gives every region's offset and
// bytes and the end: the size and the carve cannot disagree.
#pragma once
#include <stddef.h>

#include "da_sizes.hpp"
#include "pipe_carve.hpp"

namespace dagpu {

constexpr size_t kRepairCounterBytes = 256;  // kCtrSlots int32 (kernels.hpp kCtr*)

// Regions of n same-k squares, w = 2k.  Axis arrays are [axis][sq][idx].
struct RepairLayout {
  NmtCarve nmt;  // at offset 0: NMT verification (roots of the repaired square)
  WsRegion row_roots, col_roots, dah, status;  // got roots, (unused) DAHs, nmt status
  WsRegion p0;                                 // presence before repair
  WsRegion complete_before, complete_now, root_bad, parity_bad;
  WsRegion err_rows, err_cols, flags_rows, flags_cols;
  WsRegion err_share[2][2];  // [axis][key, head]
  WsRegion sel;              // exact-order repair: [2][w]
  WsRegion bits, counters;
  WsRegion fill, pair_list, pair_list_rev;  // [sq][idx] of the round's axis
  WsRegion known, deferred, nodefer, check;
  WsRegion counts[2];  // [axis] vec_counts
  size_t end;
};

inline RepairLayout repair_layout(int k, size_t n) {
  RepairLayout L{};
  const size_t w = 2 * (size_t)k;
  L.nmt = nmt_carve(k, (long)n);
  size_t p = ws_align256(L.nmt.end);
  auto take = [&](WsRegion& r, size_t want) {
    r = {p, want};
    p += ws_align256(want);
  };
  take(L.row_roots, n * w * kNodeSize);
  take(L.col_roots, n * w * kNodeSize);
  take(L.dah, n * 32);
  take(L.status, n * 4);
  take(L.p0, n * w * w);
  take(L.complete_before, n * 2 * w * 4);
  take(L.complete_now, n * 2 * w * 4);
  take(L.root_bad, n * 2 * w * 4);
  take(L.parity_bad, n * 2 * w * 4);
  take(L.err_rows, n * w * rs_err_bytes(k));
  take(L.err_cols, n * w * rs_err_bytes(k));
  take(L.flags_rows, n * w * 4);
  take(L.flags_cols, n * w * 4);
  for (int ax = 0; ax < 2; ax++)
    for (int j = 0; j < 2; j++) take(L.err_share[ax][j], n * w * 4);
  take(L.sel, 2 * w * 4);
  take(L.bits, n * 4);
  take(L.counters, kRepairCounterBytes);
  take(L.fill, n * w * 4);
  take(L.pair_list, n * w * 4);
  take(L.pair_list_rev, n * w * 4);
  take(L.known, n * 2 * w * 4);
  take(L.deferred, n * 2 * w * 4);
  take(L.nodefer, n * 4);
  take(L.check, n * 4);
  take(L.counts[0], n * w * 4);
  take(L.counts[1], n * w * 4);
  L.end = p;
  return L;
}

inline size_t repair_ws_bytes(int k, size_t n) { return repair_layout(k, n).end; }

}  // namespace dagpu
