// Stand-alone host driver of csrc/crossword_plan.hpp (tests/test_crossword_plan_host.py
// compiles and runs it; no GPU, no HIP).  Reads cases from stdin until it
// ends: k, then the (2k)^2 presence bitmap, row-major, as characters '0' / '1'
// (white space between them is skipped).  Prints for every case
//   case
//   attempt <axis> <index> <level> <orthogonal index>...     (one per attempt, in order)
//   att_level <2 * 2k values>
//   nlevels <n>
//   complete <0|1>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../celestia-app_amd/csrc/crossword_plan.hpp"

int main() {
  int k;
  while (scanf("%d", &k) == 1) {
    if (k < 1 || k > 4096) return fprintf(stderr, "bad k %d\n", k), 2;
    const size_t w = 2 * (size_t)k;
    std::vector<uint8_t> p(w * w);
    for (size_t i = 0; i < w * w; i++) {
      char c;
      if (scanf(" %c", &c) != 1 || (c != '0' && c != '1')) return fprintf(stderr, "bad bitmap\n"), 2;
      p[i] = c == '1';
    }
    const dagpu::CrossPlan pl = dagpu::plan_crossword(k, p.data());
    printf("case\n");
    for (size_t j = 0; j < pl.axis.size(); j++) {
      printf("attempt %d %d %d", pl.axis[j], pl.idx[j], pl.level[j]);
      for (int o = pl.ortho_off[j]; o < pl.ortho_off[j + 1]; o++) printf(" %d", pl.ortho[o]);
      printf("\n");
    }
    printf("att_level");
    for (int32_t v : pl.att_level) printf(" %d", v);
    printf("\nnlevels %d\ncomplete %d\n", pl.nlevels, pl.complete ? 1 : 0);
  }
  return 0;
}
