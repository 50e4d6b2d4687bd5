// crossword_plan.hpp -- rsmt2d's sequential solveCrossword order replayed on a
// presence bitmap (repair_host.cpp exact_repair decides from it which axis a
// byzantine error names).  Host arithmetic only (no HIP), so that
// tests/host/crossword_plan_check.cpp can run it without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace dagpu {

// rsmt2d solveCrossword (v0.11.0) replayed on presence bitmaps alone: the
// attempts in its sequential order (for each pass, i = 0..2k-1: row i, then
// column i; an incomplete axis with >= k shares is rebuilt), each with the
// orthogonal axes it completes (verified by rsmt2d right after the rebuild, in
// ascending index), and a dependency level: an attempt reads the cells of its
// own axis and of those orthogonal axes, so it must run after every earlier
// attempt that filled one of them.  Attempts of one level touch disjoint
// missing cells and run as one batched decode per orientation.
struct CrossPlan {
  std::vector<int> axis, idx, level;
  std::vector<int> ortho_off, ortho;  // CSR: orthogonal axes completed by attempt j
  std::vector<int32_t> att_level;     // [axis][w]: level of the axis' attempt, -1 = none
  int nlevels = 0;
  bool complete = false;              // the crossword fills the square
};

inline CrossPlan plan_crossword(int k, const uint8_t* p0) {
  const int w = 2 * k;
  CrossPlan pl;
  pl.att_level.assign(2 * (size_t)w, -1);
  std::vector<uint8_t> pres(p0, p0 + (size_t)w * w);
  std::vector<int> miss[2] = {std::vector<int>(w, 0), std::vector<int>(w, 0)};
  std::vector<int> lvl[2] = {std::vector<int>(w, -1), std::vector<int>(w, -1)};
  long missing = 0;
  for (int r = 0; r < w; r++)
    for (int c = 0; c < w; c++)
      if (!pres[(size_t)r * w + c]) { miss[0][r]++; miss[1][c]++; missing++; }
  pl.ortho_off.push_back(0);
  while (missing > 0) {
    bool progress = false;
    for (int i = 0; i < w; i++) {
      for (int ax = 0; ax < 2; ax++) {
        if (miss[ax][i] == 0 || w - miss[ax][i] < k) continue;
        int L = lvl[ax][i];
        for (int j = 0; j < w; j++) {
          const size_t cell = ax == 0 ? (size_t)i * w + j : (size_t)j * w + i;
          if (pres[cell]) continue;
          if (miss[1 - ax][j] == 1) {  // this cell is the orthogonal axis' last gap
            pl.ortho.push_back(j);
            L = std::max(L, lvl[1 - ax][j]);
          }
        }
        L += 1;
        for (int j = 0; j < w; j++) {
          const size_t cell = ax == 0 ? (size_t)i * w + j : (size_t)j * w + i;
          if (pres[cell]) continue;
          pres[cell] = 1;
          miss[ax][i]--;
          miss[1 - ax][j]--;
          lvl[1 - ax][j] = std::max(lvl[1 - ax][j], L);
          missing--;
        }
        lvl[ax][i] = std::max(lvl[ax][i], L);
        pl.axis.push_back(ax);
        pl.idx.push_back(i);
        pl.level.push_back(L);
        pl.ortho_off.push_back((int)pl.ortho.size());
        pl.att_level[(size_t)ax * w + i] = L;
        pl.nlevels = std::max(pl.nlevels, L + 1);
        progress = true;
      }
    }
    if (!progress) break;
  }
  pl.complete = missing == 0;
  return pl;
}

}  // namespace dagpu
