// Stand-alone host check of csrc/repair_layout.hpp and of the unsliced NMT
// layout in csrc/pipe_carve.hpp (tests/test_repair_layout_host.py compiles and
// runs it; no GPU, no HIP).  For k = 1, 2, 4, .., 8192 and n in {1, 2, 3, 5,
// 64, 257}, every region of both layouts
//   * starts at a multiple of 256,
//   * holds at least the bytes its users index (written out below from the
//     kernels' indexing, not taken from the header),
//   * is disjoint from every other region, and
//   * ends at or before repair_ws_bytes(k, n) / nmt_ws_bytes(k, n);
// and the regions listed here are all the regions the layout walks (their
// rounded sizes add up to its end).  Prints "k n nmt_ws_bytes repair_ws_bytes"
// per case for the Python side to compare with the recorded ABI sizes.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../celestia-app_amd/csrc/repair_layout.hpp"

using namespace dagpu;

struct Want {
  const char* name;
  WsRegion reg;
  size_t want;
};

static size_t a256(size_t v) { return (v + 255) / 256 * 256; }

// `first`: offset at which the listed regions start (they are contiguous up to `end`)
static int check(const char* what, int k, size_t n, const std::vector<Want>& regs, size_t first, size_t end) {
  size_t sum = first;
  for (size_t i = 0; i < regs.size(); i++) {
    const Want& a = regs[i];
    if (a.reg.off % 256 || a.reg.bytes < a.want || a.reg.off + a.reg.bytes > end)
      return printf("%s k=%d n=%zu: region %s [%zu, +%zu) want %zu end %zu\n", what, k, n, a.name, a.reg.off,
                    a.reg.bytes, a.want, end), 1;
    for (size_t j = 0; j < i; j++) {
      const Want& b = regs[j];
      if (a.reg.off < b.reg.off + b.reg.bytes && b.reg.off < a.reg.off + a.reg.bytes && a.reg.bytes && b.reg.bytes)
        return printf("%s k=%d n=%zu: regions %s and %s overlap\n", what, k, n, a.name, b.name), 1;
    }
    sum += a256(a.reg.bytes);
  }
  if (sum != end) return printf("%s k=%d n=%zu: listed regions end at %zu, the layout at %zu\n", what, k, n, sum, end), 1;
  return 0;
}

int main() {
  const size_t ns[] = {1, 2, 3, 5, 64, 257};
  for (int k = 1; k <= 8192; k *= 2) {
    for (size_t n : ns) {
      const size_t kk = (size_t)k, w = 2 * kk;
      // NMT (nmt.hip, nmt_forest.hip): 32-B leaf digests of every cell, 32-B
      // namespace slots of Q0, 48-B node records of levels 1 and 2 (4k trees
      // of 2k >> L nodes per square)
      const NmtCarve c = nmt_carve(k, (long)n);
      const std::vector<Want> nmt = {{"digests", c.digests, n * w * w * 32},
                                     {"ns_table", c.ns_table, n * kk * kk * 32},
                                     {"rec_a", c.rec_a, n * 2 * w * (w >> 1) * 48},
                                     {"rec_b", c.rec_b, n * 2 * w * (w >> 2) * 48}};
      if (check("nmt", k, n, nmt, 0, c.end)) return 1;
      if (c.end != nmt_ws_bytes(k, (long)n)) return printf("nmt_ws_bytes k=%d n=%zu\n", k, n), 1;

      const RepairLayout L = repair_layout(k, n);
      // error locators per vector (kernels.hpp DecodeArgs.err): GF(2^8) 256 B;
      // GF(2^16) 2k uint16 locators and 2k table images of 80 B (k <= 1024) or 32 B
      const size_t err = k <= 128 ? 256 : 4 * kk + 2 * kk * (k <= 1024 ? 80 : 32);
      const size_t vec = n * w * 4;       // one int32 per vector of one axis
      const size_t axes = n * 2 * w * 4;  // one int32 per [axis][sq][idx]
      const std::vector<Want> rep = {
          {"row_roots", L.row_roots, n * w * 90},
          {"col_roots", L.col_roots, n * w * 90},
          {"dah", L.dah, n * 32},
          {"status", L.status, n * 4},
          {"p0", L.p0, n * w * w},  // one byte per cell
          {"complete_before", L.complete_before, axes},
          {"complete_now", L.complete_now, axes},
          {"root_bad", L.root_bad, axes},
          {"parity_bad", L.parity_bad, axes},
          {"err_rows", L.err_rows, n * w * err},
          {"err_cols", L.err_cols, n * w * err},
          {"flags_rows", L.flags_rows, vec},
          {"flags_cols", L.flags_cols, vec},
          {"err_key rows", L.err_share[0][0], vec},
          {"err_head rows", L.err_share[0][1], vec},
          {"err_key cols", L.err_share[1][0], vec},
          {"err_head cols", L.err_share[1][1], vec},
          {"sel", L.sel, 2 * w * 4},  // one square's [axis][idx]
          {"bits", L.bits, n * 4},
          {"counters", L.counters, 64 * 4},  // kCtrSlots
          {"fill", L.fill, vec},
          {"pair_list", L.pair_list, vec},  // up to n * w / 2 pairs of two entries
          {"pair_list_rev", L.pair_list_rev, vec},
          {"known", L.known, axes},
          {"deferred", L.deferred, axes},
          {"nodefer", L.nodefer, n * 4},
          {"check", L.check, n * 4},
          {"counts rows", L.counts[0], vec},
          {"counts cols", L.counts[1], vec}};
      // the NMT regions come first, then the Repair regions up to the end
      if (L.nmt.end != c.end || L.row_roots.off != a256(c.end)) return printf("nmt part k=%d n=%zu\n", k, n), 1;
      if (check("repair", k, n, rep, a256(c.end), L.end)) return 1;
      if (L.end != repair_ws_bytes(k, n)) return printf("repair_ws_bytes k=%d n=%zu\n", k, n), 1;
      printf("%d %zu %zu %zu\n", k, n, c.end, L.end);
    }
  }
  return 0;
}
