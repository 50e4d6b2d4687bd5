// Stand-alone host check of csrc/ns_find.hpp (tests/test_ns_find_host.py
// compiles and runs it; no GPU, no HIP, no Python in the process).
//   * For every row of 1 .. 16 leaves and every sorted multiset of namespaces
//     over 3 distinct values: ns_find equals a linear scan for the values, the
//     gaps between them and both ends; the root's range is the first and the
//     last leaf, and once more with the last value taken as a parity half that
//     the root's max ignores.
//   * The returned range is always inside the row, and a leaf is only read at
//     an index below the row length.
//   * ns_key_bytes orders keys as memcmp orders the 29 bytes.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../celestia-app_amd/csrc/ns_find.hpp"

using namespace dagpu;

// v = 0 .. 8, increasing bytewise; the deciding byte lies in a different key word each time
static void make_ns(uint8_t* p, int v) {
  memset(p, 0, 29);
  switch (v) {
    case 0: break;
    case 1: p[28] = 1; break;
    case 2: p[20] = 1; break;
    case 3: p[20] = 1; p[25] = 7; break;
    case 4: p[8] = 1; break;
    case 5: p[0] = 1; break;
    case 6: memset(p, 0xFF, 28); p[28] = 0xF6; break;
    case 7: memset(p, 0xFF, 28); p[28] = 0xFE; break;
    default: memset(p, 0xFF, 29); break;
  }
}

static int fail(const char* what, long a = 0, long b = 0, long c = 0) {
  printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
  return 1;
}

int main() {
  // keys order as the bytes do
  long ordered = 0;
  for (int a = 0; a <= 8; a++)
    for (int b = 0; b <= 8; b++) {
      uint8_t x[29], y[29];
      make_ns(x, a);
      make_ns(y, b);
      const bool less = memcmp(x, y, 29) < 0;
      if (ns_key_less(ns_key_bytes(x), ns_key_bytes(y)) != less) return fail("key order", a, b);
      if (less != (a < b)) return fail("test namespaces are not increasing", a, b);
      ordered++;
    }
  // leaf values 1, 3, 5 (and 8 = parity in the second pass); queries 0 .. 8
  long rows = 0, checks = 0, kinds[3] = {0, 0, 0};
  for (int pass = 0; pass < 2; pass++) {
    const int vals[3] = {1, 3, pass == 0 ? 5 : 8};
    for (uint32_t n = 1; n <= 16; n++)
      for (uint32_t c0 = 0; c0 <= n; c0++)
        for (uint32_t c1 = 0; c0 + c1 <= n; c1++) {
          const uint32_t c2 = n - c0 - c1;
          std::vector<int> leaf(n);
          for (uint32_t i = 0; i < n; i++) leaf[i] = i < c0 ? vals[0] : i < c0 + c1 ? vals[1] : vals[2];
          // root: min = first leaf; max = last leaf, the parity half ignored unless it is the whole row
          int rmin = leaf[0], rmax = leaf[n - 1];
          if (pass == 1 && c2 > 0 && c2 < n) rmax = leaf[n - c2 - 1];
          uint8_t b[29];
          make_ns(b, rmin);
          const NsKey kmin = ns_key_bytes(b);
          make_ns(b, rmax);
          const NsKey kmax = ns_key_bytes(b);
          rows++;
          for (int q = 0; q <= 8; q++) {
            // linear scan
            int want = kNsOutside;
            uint32_t ws = 0, we = 0;
            if (!(q < rmin || rmax < q)) {
              uint32_t s = n, e = n;
              for (uint32_t i = 0; i < n; i++) {
                if (leaf[i] >= q && s == n) s = i;
                if (leaf[i] > q && e == n) e = i;
              }
              if (e > s) { want = kNsPresent; ws = s; we = e; }
              else { want = kNsAbsent; ws = s; we = s + 1; }
            }
            make_ns(b, q);
            bool past = false;
            uint32_t s = 99, e = 99;
            const int got = ns_find(ns_key_bytes(b), kmin, kmax, n,
                                    [&](uint32_t i) {
                                      if (i >= n) { past = true; i = n - 1; }
                                      uint8_t t[29];
                                      make_ns(t, leaf[i]);
                                      return ns_key_bytes(t);
                                    },
                                    &s, &e);
            if (past) return fail("leaf read past the row", n, q);
            if (s > e || e > n) return fail("range outside the row", n, s, e);
            if (got != want || s != ws || e != we) return fail("ns_find differs from the scan", n, q, got);
            kinds[got]++;
            checks++;
          }
        }
  }
  // a root that claims more than its leaves hold: answered as outside, no index past the row
  {
    uint8_t b[29];
    make_ns(b, 1);
    const NsKey k1 = ns_key_bytes(b);
    make_ns(b, 5);
    const NsKey k5 = ns_key_bytes(b);
    make_ns(b, 3);
    uint32_t s = 99, e = 99;
    if (ns_find(ns_key_bytes(b), k1, k5, 4, [&](uint32_t) { return k1; }, &s, &e) != kNsOutside || s || e)
      return fail("inconsistent root");
  }
  printf("OK ordered=%ld rows=%ld checks=%ld outside=%ld present=%ld absent=%ld\n", ordered, rows, checks, kinds[0],
         kinds[1], kinds[2]);
  return 0;
}
