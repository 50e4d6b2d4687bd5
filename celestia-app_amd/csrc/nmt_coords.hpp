// nmt_coords.hpp -- index maps of the NMT leaf and tree-level kernels (nmt.hip):
// (workgroup, lane) -> (square, cell) and (square, axis, tree, node), and from
// there to digest / record indices.  No HIP types, so tests/host/
// nmt_coords_check.cpp compiles it with a host compiler and pins the maps
// against the division formulas they replaced.
//
// The layouts are those of nmt.hip and pipe_carve.hpp, unchanged: a square's
// leaf digests are row-major cells (32 B); its level-L records (48 B) are
// [row trees: w x per, tree-major][column trees: per x w, NODE-major] with
// per = w >> L; the Q0 namespace table is k x k entries of 32 B.
//
// w = 2k is a power of two, so every division is a shift and every remainder a
// mask; the shift counts (Leaf/LevelMap) are kernel arguments.  Workgroups have
// 256 lanes and the grid is one-dimensional: square, axis and block-in-axis are
// bit fields of blockIdx.x (batches or widths beyond a 65,535-block y or z
// dimension are therefore folded into x, whose limit of 2^31 - 1 blocks the
// launchers check).  Two shapes of map:
//
//   wide   a (square, axis) of a level, or a square's cells of a leaf launch,
//          has >= 256 lanes of work: a workgroup lies inside one of them.
//          Square, axis and the workgroup's first item come from blockIdx.x
//          alone (scalar registers); a lane adds threadIdx.x.  Every byte
//          address is a 64-bit block-uniform base plus a 32-bit lane offset:
//            leaf      eds: lane * 512 < 2^17,  digest: lane * 32 < 2^13,
//                      ns_table: (r * k + c) * 32 < 2^31     (k <= 8192)
//            level     out: lane * 48 < 2^14,  left child: < 512 * 48 < 2^15,
//                      right child: 48 B (rows) or w * 48 < 2^20 B (columns) on,
//                      ns_table by reference: ref * 32 < 2^31 (k <= 8192)
//          so the row of a cell (whose byte offset in its square passes 2^32
//          at k = 8192) is always in the scalar part.
//   small  fewer than 256 lanes per square (leaf launches of k <= 8, levels
//          near the top, every level of k <= 8): 256 >> log2(items per square)
//          squares share a workgroup; the square index is per lane and the
//          addresses take one 64-bit multiply-add per lane.  Lanes past the
//          last square are idle.
//
// Both shapes give lane (blockIdx.x, threadIdx.x) the item of flat index
// blockIdx.x * 256 + threadIdx.x in [square][axis][record] order (leaves, with
// a power-of-two row count: [square][cell]), the order of the former maps, so
// a level's output record index is that flat index.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NMT_HD __host__ __device__ __forceinline__
#else
#define NMT_HD inline
#endif

namespace dagpu {

constexpr int kNmtBlockLog = 8;  // 256-lane workgroups
constexpr long kNmtMaxBlocks = 0x7FFFFFFFL;
constexpr int kNmtMaxK = 8192;  // ref * 32 and (r * k + c) * 32 stay below 2^32

// log2 of a power of two, -1 for anything else
inline int nmt_log2(long v) {
  if (v <= 0 || (v & (v - 1))) return -1;
  int l = 0;
  while ((1L << l) < v) l++;
  return l;
}

// ---------------------------------------------------------------------------
// Leaves: a launch covers rows [row0, row0 + nrows) of every square.  A square
// takes 2^ls lane slots, ls = lw + log2(nrows rounded up to a power of two);
// slot s is cell row0 * w + s of the square, idle when s >= nrows * w.
// ---------------------------------------------------------------------------
struct LeafMap {
  int lw;          // log2(w)
  int ls;          // log2(lane slots per square)
  uint32_t cell0;  // row0 * w
  uint32_t ncell;  // nrows * w
  long nsq;
};

inline bool leaf_map(int k, long nsq, int row0, int nrows, LeafMap& m) {
  const int lk = nmt_log2(k);
  if (lk < 0 || k > kNmtMaxK || nsq <= 0 || row0 < 0 || nrows <= 0 || row0 + nrows > 2 * k) return false;
  int lp = 0;
  while ((1 << lp) < nrows) lp++;
  m.lw = lk + 1;
  m.ls = m.lw + lp;
  m.cell0 = (uint32_t)row0 << m.lw;
  m.ncell = (uint32_t)nrows << m.lw;
  m.nsq = nsq;
  return true;
}

inline bool leaf_wide(const LeafMap& m) { return m.ls >= kNmtBlockLog; }

// workgroups of the launch (the launcher refuses more than kNmtMaxBlocks)
inline long leaf_blocks(const LeafMap& m) {
  if (leaf_wide(m)) return m.nsq << (m.ls - kNmtBlockLog);
  const int q = kNmtBlockLog - m.ls;  // log2(squares per workgroup)
  return (m.nsq + (1L << q) - 1) >> q;
}

struct LeafCell {
  long sq;          // wide: block-uniform
  uint32_t cell_u;  // block-uniform part of the cell index in the square (< 2^30)
  uint32_t lane;    // per-lane part (< 256): cell = cell_u + lane
  bool valid;
};

template <bool kWide>
NMT_HD LeafCell leaf_cell(const LeafMap& m, uint32_t bx, uint32_t tid) {
  LeafCell c;
  if constexpr (kWide) {
    const int sh = m.ls - kNmtBlockLog;
    c.sq = (long)(bx >> sh);
    const uint32_t s0 = (bx & ((1u << sh) - 1u)) << kNmtBlockLog;
    c.cell_u = m.cell0 + s0;
    c.lane = tid;
    c.valid = s0 + tid < m.ncell;
  } else {
    c.sq = ((long)bx << (kNmtBlockLog - m.ls)) + (tid >> m.ls);
    c.cell_u = m.cell0;
    c.lane = tid & ((1u << m.ls) - 1u);
    c.valid = c.sq < m.nsq && c.lane < m.ncell;
  }
  return c;
}

NMT_HD uint32_t leaf_row(const LeafMap& m, const LeafCell& c) { return (c.cell_u + c.lane) >> m.lw; }
NMT_HD uint32_t leaf_col(const LeafMap& m, const LeafCell& c) { return (c.cell_u + c.lane) & ((1u << m.lw) - 1u); }

// ---------------------------------------------------------------------------
// Tree levels.  Level L (1 .. lw) has per = w >> L nodes per tree and
// A = w * per = 2^la nodes per (square, axis).  Node g (0 .. A) of an axis is
//   rows:     tree g >> (la - lw), node g & (per - 1)      (tree-major)
//   columns:  node g >> lw,        tree g & (w - 1)        (node-major)
// Its children are items 2 * node and 2 * node + 1 of the same tree one level
// down (level 0: the leaf digests, both axes over the same row-major cells).
// Relative to the axis' first item there that is
//   rows:     2 g, 2 g + 1                  (adjacent)
//   columns:  g + (g >> lw) * w, ... + w    (one row of w items apart)
// and with g = g_u + lane, g_u a multiple of 256 (wide) or 0 (small), the
// column form splits into (g_u + (g_u >> lw) * w) + (lane + (lane >> lw) * w):
// for w >= 256 the lane term is just lane, for w < 256 w divides g_u.
// ---------------------------------------------------------------------------
struct LevelMap {
  int lw;  // log2(w)
  int la;  // log2(A) = 2 lw - L
  long nsq;
};

inline bool level_map(int k, long nsq, int level, LevelMap& m) {
  const int lk = nmt_log2(k);
  if (lk < 0 || k > kNmtMaxK || nsq <= 0 || level < 1 || level > lk + 1) return false;
  m.lw = lk + 1;
  m.la = 2 * m.lw - level;
  m.nsq = nsq;
  return true;
}

inline bool level_wide(const LevelMap& m) { return m.la >= kNmtBlockLog; }

inline long level_blocks(const LevelMap& m) {
  if (level_wide(m)) return m.nsq << (m.la + 1 - kNmtBlockLog);
  const int q = kNmtBlockLog - (m.la + 1);  // log2(squares per workgroup)
  return (m.nsq + (1L << q) - 1) >> q;
}

struct LevelNode {
  long sq;        // wide: block-uniform
  uint32_t axis;  // 0 rows, 1 columns; wide: block-uniform
  uint32_t g_u;   // block-uniform part of the node's index in its axis (< 2^27)
  uint32_t lane;  // per-lane part (< 256): g = g_u + lane
  bool valid;
};

template <bool kWide>
NMT_HD LevelNode level_node(const LevelMap& m, uint32_t bx, uint32_t tid) {
  LevelNode n;
  if constexpr (kWide) {
    const int sh = m.la - kNmtBlockLog;
    n.sq = (long)(bx >> (sh + 1));
    n.axis = (bx >> sh) & 1u;
    n.g_u = (bx & ((1u << sh) - 1u)) << kNmtBlockLog;
    n.lane = tid;
    n.valid = true;
  } else {
    n.sq = ((long)bx << (kNmtBlockLog - (m.la + 1))) + (tid >> (m.la + 1));
    n.axis = (tid >> m.la) & 1u;
    n.g_u = 0;
    n.lane = tid & ((1u << m.la) - 1u);
    n.valid = n.sq < m.nsq;
  }
  return n;
}

// tree (row or column index) and node within the tree
NMT_HD uint32_t level_tree(const LevelMap& m, const LevelNode& n) {
  const uint32_t g = n.g_u + n.lane;
  return n.axis == 0 ? g >> (m.la - m.lw) : g & ((1u << m.lw) - 1u);
}
NMT_HD uint32_t level_pos(const LevelMap& m, const LevelNode& n) {
  const uint32_t g = n.g_u + n.lane;
  return n.axis == 0 ? g & ((1u << (m.la - m.lw)) - 1u) : g >> m.lw;
}

// Output record of the node, counted from the launch's first record
// (== sq * 2A + axis * A + g): block part and lane part.
NMT_HD long level_out_u(uint32_t bx) { return (long)bx << kNmtBlockLog; }
NMT_HD uint32_t level_out_l(uint32_t tid) { return tid; }

// Left child, counted in items (records; level 1: cells) from the launch's
// first item one level down: block part and lane part.  The right child is
// level_child_step items further.
NMT_HD long level_child_u(const LevelMap& m, const LevelNode& n, bool level1) {
  const long sq_items = level1 ? n.sq << (m.la + 1) : n.sq << (m.la + 2);
  const long axis_items = level1 ? 0L : (long)n.axis << (m.la + 1);
  const uint32_t g = n.axis == 0 ? 2u * n.g_u : n.g_u + ((n.g_u >> m.lw) << m.lw);
  return sq_items + axis_items + g;
}
NMT_HD uint32_t level_child_l(const LevelMap& m, const LevelNode& n) {
  return n.axis == 0 ? 2u * n.lane : n.lane + ((n.lane >> m.lw) << m.lw);
}
NMT_HD uint32_t level_child_step(const LevelMap& m, const LevelNode& n) { return n.axis == 0 ? 1u : 1u << m.lw; }

}  // namespace dagpu
