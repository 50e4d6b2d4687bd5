// Stand-alone host check of csrc/pipe_carve.hpp (tests/test_pipe_carve_host.py
// compiles and runs it; no GPU, no HIP).  For every k in 1..512, n in 1..300,
// S in 1..8 and every cut level (the rule's own choice included):
//   * when the carve reports `defer`, its six regions are pairwise disjoint,
//     hold what their users address, and end at or before
//     dagpu_workspace_size(k, n);
//   * when it does not, the regions really cannot fit (or nothing is deferred).
// The sizes are recomputed here from the record formats, not taken from the header.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../celestia-app_amd/csrc/pipe_carve.hpp"

using namespace dagpu;

static size_t a256(size_t v) { return (v + 255) / 256 * 256; }

// dagpu_workspace_size(k, n): digests, Q0 namespaces, level-1 and level-2 records of n squares + 256
static size_t workspace_size(size_t k, size_t n) {
  const size_t w = 2 * k;
  return a256(w * w * 32 * n) + a256(k * k * 32 * n) + a256(n * 2 * w * (w / 2) * 48) +
         a256(n * 2 * w * std::max<size_t>(w / 4, 1) * 48) + 256;
}

static size_t rec_bytes(size_t k, int L) { return 2 * (2 * k) * ((2 * k) >> L) * 48; }

int main() {
  long checked = 0, deferred = 0, fallback = 0;
  for (int k = 1; k <= 512; k++) {
    int levels = 0;
    while ((1 << levels) < 2 * k) levels++;
    if (levels != nmt_levels(k)) return printf("levels k=%d\n", k), 1;
    for (size_t n = 1; n <= 300; n++) {
      const size_t limit = workspace_size(k, n);
      if (limit != nmt_ws_bytes(k, (long)n) + 256) return printf("workspace size k=%d n=%zu\n", k, n), 1;
      for (size_t S = 1; S <= 8; S++) {
        size_t m = 0;  // largest of the cuts n * i / S
        for (size_t i = 0; i < S; i++) m = std::max(m, n * (i + 1) / S - n * i / S);
        const int rule = pipe_cut_level(k, m, 1280);
        if (rule < 1 || rule > levels) return printf("rule k=%d n=%zu S=%zu: %d\n", k, n, S, rule), 1;
        for (int cut = 0; cut <= levels + 1; cut++) {
          const PipeCarve c = pipe_carve(k, n, m, cut, limit);
          checked++;
          const size_t kk = (size_t)k, w = 2 * kk;
          // what the launches address: slice regions for m squares, batch regions for n
          const size_t want[6] = {w * w * 32 * m,  m * rec_bytes(kk, 1), m * rec_bytes(kk, 2),
                                  kk * kk * 32 * n, n * rec_bytes(kk, cut < 0 ? 0 : cut), n * rec_bytes(kk, cut + 1)};
          if (!c.defer) {
            fallback++;
            const bool nothing = cut < 1 || cut >= levels || m >= n;
            size_t need = 0;
            for (size_t b : want) need += a256(b);
            if (!nothing && need <= limit)
              return printf("k=%d n=%zu S=%zu cut=%d: fits (%zu <= %zu) but reported the fallback\n", k, n, S, cut,
                            need, limit), 1;
            continue;
          }
          deferred++;
          if (S < 2 || cut < 1 || cut >= levels) return printf("k=%d n=%zu S=%zu cut=%d: deferred\n", k, n, S, cut), 1;
          const std::pair<size_t, size_t> reg[6] = {{c.digests, c.digests_bytes}, {c.rec_a, c.rec_a_bytes},
                                                    {c.rec_b, c.rec_b_bytes},     {c.ns_all, c.ns_all_bytes},
                                                    {c.rec_c, c.rec_c_bytes},     {c.rec_d, c.rec_d_bytes}};
          for (int i = 0; i < 6; i++) {
            if (reg[i].second < want[i] || reg[i].first % 256 || reg[i].first + reg[i].second > limit ||
                reg[i].first + reg[i].second > c.end || c.end > limit)
              return printf("k=%d n=%zu S=%zu cut=%d: region %d [%zu, +%zu) want %zu limit %zu\n", k, n, S, cut, i,
                            reg[i].first, reg[i].second, want[i], limit), 1;
            for (int j = 0; j < i; j++)
              if (reg[i].first < reg[j].first + reg[j].second && reg[j].first < reg[i].first + reg[i].second &&
                  reg[i].second && reg[j].second)
                return printf("k=%d n=%zu S=%zu cut=%d: regions %d and %d overlap\n", k, n, S, cut, i, j), 1;
          }
        }
      }
    }
  }
  printf("ok checked=%ld deferred=%ld fallback=%ld\n", checked, deferred, fallback);
  return 0;
}
