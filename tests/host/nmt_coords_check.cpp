// Stand-alone host check of csrc/nmt_coords.hpp (tests/test_nmt_coords_host.py
// compiles and runs it; no GPU, no HIP).  The shift-and-mask maps of the NMT
// leaf and level kernels are pinned against the division formulas the kernels
// used before (old_* below, copied from that nmt.hip):
//   * for every power of two k in 1..512, n in {1, 2, 3}, the three leaf
//     launches of the pipeline (all rows; rows 0..k-1; rows k..2k-1) and every
//     tree level, lane (block, thread) of the new map holds exactly the item of
//     flat index block * 256 + thread of the old map; every item is enumerated
//     once and nothing lies out of range;
//   * byte offsets (share, digest, Q0 namespace entry, child and output
//     records) equal the old 64-bit ones, record indices equal level_rec's;
//   * in the wide shape, square, axis and the block parts depend on the block
//     index alone, and the lane parts respect the bounds the header states;
//   * leaf launches over a row count that is no power of two enumerate the
//     same set of cells as the old map (their order differs);
//   * sampled workgroups at k = 8192 check the 32-bit bounds where a cell's
//     byte offset in its square passes 2^32.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../celestia-app_amd/csrc/nmt_coords.hpp"

using namespace dagpu;

#define CHECK(c, ...)                          \
  do {                                         \
    if (!(c)) {                                \
      printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                     \
      printf("\n");                            \
      return false;                            \
    }                                          \
  } while (0)

// --- the former maps ---------------------------------------------------------
static void old_level_coords(long gid, int w, int per, long& sq, int& axis, int& idx, int& p) {
  const long blk = 2L * w * per;
  sq = gid / blk;
  const long g = gid - sq * blk;
  axis = g >= (long)w * per;
  const long g2 = g - (axis ? (long)w * per : 0);
  if (axis == 0) { idx = (int)(g2 / per); p = (int)(g2 - (long)idx * per); }
  else { p = (int)(g2 / w); idx = (int)(g2 - (long)p * w); }
}

static long old_level_rec(long sq, int w, int per, int axis, int idx, int p) {
  const long base = sq * 2L * w * per;
  return axis == 0 ? base + (long)idx * per + p : base + (long)w * per + (long)p * w + idx;
}

static void old_leaf(long gid, long w, int row0, int nrows, long& sq, long& cell) {
  const long span = nrows * w;
  sq = gid / span;
  cell = row0 * w + (gid - sq * span);
}

static long g_leaves = 0, g_nodes = 0, g_sampled = 0;

// one lane of a leaf launch against the old byte offsets; `flat` < 0: no old lane to compare the order with
static bool check_leaf_lane(const LeafMap& m, int k, long stride, uint32_t bx, uint32_t tid, long flat, int row0,
                            int nrows, long& sq_out, long& cell_out) {
  const long w = 2L * k;
  const bool wide = leaf_wide(m);
  const LeafCell c = wide ? leaf_cell<true>(m, bx, tid) : leaf_cell<false>(m, bx, tid);
  sq_out = -1;
  if (!c.valid) return true;
  CHECK(c.lane < 256, "leaf lane part %u", c.lane);
  if (wide) {
    const LeafCell c0 = leaf_cell<true>(m, bx, 0);
    CHECK(c0.sq == c.sq && c0.cell_u == c.cell_u && c.lane == tid, "leaf block parts vary in block %u", bx);
  }
  const long cell = (long)c.cell_u + c.lane;
  const uint32_t r = leaf_row(m, c), col = leaf_col(m, c);
  CHECK(c.sq >= 0 && c.sq < m.nsq, "leaf square %ld", c.sq);
  CHECK(r == cell / w && col == cell % w, "leaf row/col k=%d cell=%ld", k, cell);
  CHECK((long)r >= row0 && (long)r < row0 + nrows, "leaf row %u outside [%d, %d)", r, row0, row0 + nrows);
  if (flat >= 0) {
    long osq, ocell;
    old_leaf(flat, w, row0, nrows, osq, ocell);
    CHECK(osq == c.sq && ocell == cell, "leaf k=%d flat=%ld: (%ld, %ld) != old (%ld, %ld)", k, flat, c.sq, cell, osq,
          ocell);
  }
  // byte offsets as the kernel forms them: 64-bit block part + 32-bit lane part
  const int lk = m.lw - 1;
  const long src = c.sq * stride + (long)c.cell_u * 512 + (long)(uint32_t)(c.lane * 512u);
  CHECK(src == c.sq * stride + cell * 512, "leaf share offset");
  const long dig = ((c.sq << (2 * m.lw)) + c.cell_u) * 32 + (long)(uint32_t)(c.lane * 32u);
  CHECK(dig == (c.sq * w * w + cell) * 32, "leaf digest offset");
  if ((long)r < k && (long)col < k) {
    CHECK(((r | col) >> lk) == 0, "q0 test");
    const long ns = (c.sq << (2 * lk + 5)) + (long)(uint32_t)(((r << lk) + col) << 5);
    CHECK(ns == (c.sq * k * k + (long)r * k + col) * 32, "leaf namespace offset");
  } else {
    CHECK(((r | col) >> lk) != 0, "q0 test");
  }
  sq_out = c.sq;
  cell_out = cell;
  return true;
}

static bool check_leaves(int k, long nsq, int row0, int nrows) {
  const long w = 2L * k, cells = w * w, stride = cells * 512 + 4096;  // any stride >= the square
  LeafMap m;
  CHECK(leaf_map(k, nsq, row0, nrows, m), "leaf_map k=%d", k);
  const bool pow2 = nmt_log2(nrows) >= 0;
  const long total = nrows * w * nsq, blocks = leaf_blocks(m);
  CHECK(blocks > 0 && blocks <= kNmtMaxBlocks, "leaf blocks");
  if (pow2) CHECK(blocks == (total + 255) / 256, "leaf blocks %ld, old %ld", blocks, (total + 255) / 256);
  std::vector<uint8_t> seen((size_t)(nsq * cells), 0);
  long count = 0;
  for (long bx = 0; bx < blocks; bx++)
    for (uint32_t tid = 0; tid < 256; tid++) {
      const long flat = bx * 256 + tid;
      long sq, cell;
      if (!check_leaf_lane(m, k, stride, (uint32_t)bx, tid, pow2 && flat < total ? flat : -1, row0, nrows, sq, cell))
        return false;
      if (pow2) CHECK((sq >= 0) == (flat < total), "leaf k=%d lane %ld validity", k, flat);
      if (sq < 0) continue;
      CHECK(!seen[(size_t)(sq * cells + cell)], "leaf k=%d cell twice", k);
      seen[(size_t)(sq * cells + cell)] = 1;
      count++;
    }
  CHECK(count == total, "leaf k=%d: %ld lanes, old %ld", k, count, total);
  for (long gid = 0; gid < total; gid++) {  // the old map's set is covered
    long sq, cell;
    old_leaf(gid, w, row0, nrows, sq, cell);
    CHECK(seen[(size_t)(sq * cells + cell)], "leaf k=%d old cell not covered", k);
  }
  g_leaves += count;
  return true;
}

static bool check_level_lane(const LevelMap& m, int k, int L, uint32_t bx, uint32_t tid, bool& valid) {
  const int w = 2 * k, per = w >> L;
  const bool wide = level_wide(m);
  const LevelNode n = wide ? level_node<true>(m, bx, tid) : level_node<false>(m, bx, tid);
  valid = n.valid;
  if (!n.valid) return true;
  const long gid = (long)bx * 256 + tid;
  long sq;
  int axis, idx, p;
  old_level_coords(gid, w, per, sq, axis, idx, p);
  CHECK(n.sq >= 0 && n.sq < m.nsq, "level square %ld", n.sq);
  CHECK(n.sq == sq && (int)n.axis == axis && (int)level_tree(m, n) == idx && (int)level_pos(m, n) == p,
        "level k=%d L=%d gid=%ld: (%ld, %u, %u, %u) != old (%ld, %d, %d, %d)", k, L, gid, n.sq, n.axis,
        level_tree(m, n), level_pos(m, n), sq, axis, idx, p);
  CHECK(idx < w && p < per, "level coordinates out of range");
  CHECK(n.lane < 256 && n.g_u < (1u << 27), "level lane / block parts");
  const long cu = level_child_u(m, n, L == 1);
  const uint32_t cl = level_child_l(m, n), step = level_child_step(m, n);
  CHECK(cl < 512 && (uint64_t)(cl + step) * 48 < (1u << 20), "child lane part %u", cl);
  if (wide) {
    const LevelNode n0 = level_node<true>(m, bx, 0);
    CHECK(n0.sq == n.sq && n0.axis == n.axis && n0.g_u == n.g_u && n.lane == tid &&
              level_child_u(m, n0, L == 1) == cu && level_child_step(m, n0) == step,
          "level block parts vary in block %u", bx);
  }
  CHECK(level_out_u(bx) + level_out_l(tid) == old_level_rec(sq, w, per, axis, idx, p), "output record");
  if (L == 1) {  // children: cells 2p, 2p + 1 of row / column idx
    const long j0 = 2L * p, j1 = j0 + 1;
    const long cell0 = axis == 0 ? (long)idx * w + j0 : j0 * w + idx;
    const long cell1 = axis == 0 ? (long)idx * w + j1 : j1 * w + idx;
    CHECK(cu + cl == sq * w * w + cell0 && cu + cl + step == sq * w * w + cell1, "level-1 children");
  } else {
    CHECK(cu + cl == old_level_rec(sq, w, 2 * per, axis, idx, 2 * p) &&
              cu + cl + step == old_level_rec(sq, w, 2 * per, axis, idx, 2 * p + 1),
          "level k=%d L=%d gid=%ld children", k, L, gid);
    const int lk = m.lw - 1;
    CHECK((n.sq << (2 * m.lw + 3)) == n.sq * k * k * 32 && (n.sq << (2 * lk + 5)) == n.sq * k * k * 32, "ns base");
  }
  return true;
}

static bool check_level(int k, long nsq, int L) {
  const int w = 2 * k, per = w >> L;
  LevelMap m;
  CHECK(level_map(k, nsq, L, m), "level_map k=%d L=%d", k, L);
  const long total = nsq * 2L * w * per, blocks = level_blocks(m);
  CHECK(blocks == (total + 255) / 256, "level blocks %ld, old %ld", blocks, (total + 255) / 256);
  // flat index == old gid for every lane, so each record is enumerated once iff
  // the valid lanes are exactly gid < total
  for (long bx = 0; bx < blocks; bx++)
    for (uint32_t tid = 0; tid < 256; tid++) {
      bool valid;
      if (!check_level_lane(m, k, L, (uint32_t)bx, tid, valid)) return false;
      CHECK(valid == (bx * 256 + tid < total), "level k=%d L=%d validity", k, L);
    }
  g_nodes += total;
  return true;
}

// k = 8192: a cell's byte offset in its square passes 2^32, a level's records 2^32 bytes
static bool check_sampled_8192() {
  const int k = 8192;
  const long nsq = 2, w = 2L * k, stride = w * w * 512;
  uint64_t x = 88172645463325252ull;
  auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  const int shapes[3][2] = {{0, 2 * k}, {0, k}, {k, k}};
  for (auto& sh : shapes) {
    LeafMap m;
    CHECK(leaf_map(k, nsq, sh[0], sh[1], m) && leaf_wide(m), "leaf_map 8192");
    const long blocks = leaf_blocks(m);
    CHECK(blocks == sh[1] * w * nsq / 256, "leaf blocks 8192");
    for (int i = 0; i < 2000; i++) {
      const long bx = i == 0 ? 0 : i == 1 ? blocks - 1 : (long)(rnd() % (uint64_t)blocks);
      for (uint32_t tid = 0; tid < 256; tid += (i < 2 ? 1 : 85)) {
        long sq, cell;
        if (!check_leaf_lane(m, k, stride, (uint32_t)bx, tid, bx * 256 + tid, sh[0], sh[1], sq, cell)) return false;
        CHECK(sq >= 0, "valid");
        g_sampled++;
      }
    }
    const LeafCell last = leaf_cell<true>(m, (uint32_t)(blocks - 1), 255);
    CHECK((long)last.cell_u * 512 > (1L << 32) && last.lane * 512u < (1u << 17), "the row is in the scalar part");
  }
  CHECK((((uint64_t)k * k - 1) << 5) < (1ull << 32), "namespace reference offset fits 32 bits");
  for (int L = 1; L <= 14; L++) {
    LevelMap m;
    CHECK(level_map(k, nsq, L, m) && level_wide(m), "level_map 8192");
    const long blocks = level_blocks(m);
    for (int i = 0; i < 2000; i++) {
      const long bx = i == 0 ? 0 : i == 1 ? blocks - 1 : (long)(rnd() % (uint64_t)blocks);
      for (uint32_t tid = 0; tid < 256; tid += (i < 2 ? 1 : 85)) {
        bool valid;
        if (!check_level_lane(m, k, L, (uint32_t)bx, tid, valid)) return false;
        CHECK(valid, "valid");
        g_sampled++;
      }
    }
  }
  return true;
}

int main() {
  LeafMap lm;
  LevelMap vm;
  for (int k : {0, 3, 6, 12, 100, 16384})  // not a power of two, or wider than the 32-bit bounds allow
    if (leaf_map(k, 1, 0, 1, lm) || level_map(k, 1, 1, vm)) return printf("FAIL k=%d accepted\n", k), 1;
  if (leaf_map(8, 1, 9, 8, lm) || leaf_map(8, 1, 0, 0, lm) || level_map(8, 1, 5, vm) || level_map(8, 1, 0, vm))
    return printf("FAIL bad rows / level accepted\n"), 1;
  for (int k = 1; k <= 512; k *= 2)
    for (long n = 1; n <= 3; n++) {
      if (!check_leaves(k, n, 0, 2 * k) || !check_leaves(k, n, 0, k) || !check_leaves(k, n, k, k)) return 1;
      int levels = 0;
      while ((1 << levels) < 2 * k) levels++;
      for (int L = 1; L <= levels; L++)
        if (!check_level(k, n, L)) return 1;
      if (k >= 2 && k <= 64)  // row counts that are no power of two
        if (!check_leaves(k, n, 1, 2 * k - 1) || !check_leaves(k, n, k - 1, 3)) return 1;
    }
  // many small squares in one workgroup, the last one partly idle
  for (long n : {63L, 64L, 65L, 1000L})
    if (!check_leaves(1, n, 0, 2) || !check_leaves(2, n, 0, 2) || !check_level(1, n, 1) || !check_level(4, n, 3))
      return 1;
  if (!check_sampled_8192()) return 1;
  printf("ok leaves=%ld nodes=%ld sampled=%ld\n", g_leaves, g_nodes, g_sampled);
  return 0;
}
