// forest.hpp -- generic batched Merkle forests (nmt_forest.hip) and the host
// planner that lays out their levels.  See nmt_forest.hip for the semantics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "kernels.hpp"

namespace dagpu {

// leaf prefix modes
constexpr int kPfxNone = 0;    // message 0x00 | data (plain nmt Push / RFC-6962 item)
constexpr int kPfxSelf = 1;    // 0x00 | data[0:29] | data   (wrapper Q0, blob commitment)
constexpr int kPfxParity = 2;  // 0x00 | 0xFF*29 | data      (wrapper Q1..Q3)
constexpr int kPfxFlags = 3;   // per-leaf kPfxSelf / kPfxParity byte
constexpr int kPfxGrid = 4;    // wrapper rule by cell coordinates (row<k && col<k -> self)

constexpr int kRecNmt = 96;    // minNs[32] | maxNs[32] | digest[32]
constexpr int kRecRfc = 32;    // digest

// Per-tree status bit (nmt ErrInvalidPushOrder).
constexpr int kForestPushOrder = 1;

struct ForestLeafArgs {
  const uint8_t* data;
  long data_stride;  // bytes between consecutive leaves (multiple of 4)
  long dlen;         // data bytes per leaf
  long nleaves;
  int pmode;
  const uint8_t* pflags;          // kPfxFlags
  int grid_k;                     // kPfxGrid: original square width
  long grid_w, grid_r0, grid_c0;  // leaf i = cell (r0 + i / w, c0 + i % w)
  int rfc;                        // 1: RFC-6962 leaf digest, 0: NMT leaf record
  uint8_t* out;                   // nleaves records
};

struct ForestLevelArgs {
  const uint8_t* in;
  uint8_t* out;
  // input node j of tree t: in + (base(t) + j * in_lstride) * rec, where
  // base(t) = in_off ? in_off[t] : t * in_tstride and count(t) = in_off ?
  // in_off[t+1] - in_off[t] : in_per.
  const int64_t* in_off;
  long in_tstride, in_lstride, in_per;
  // output node j of tree t: out + (obase(t) + j) * rec, obase(t) = out_off ?
  // out_off[t] : t * out_per
  const int64_t* out_off;
  long out_per;
  long ntrees, total_out;
  int ignore_max, check_order, rfc;
  int32_t* status;  // per tree, OR kForestPushOrder (check_order only)
  int status_shared;  // 1: every tree ORs into status[0] (one flag for the batch)
};

hipError_t launch_forest_leaves(const ForestLeafArgs& a, hipStream_t s);
hipError_t launch_forest_level(const ForestLevelArgs& a, hipStream_t s);
// roots: root_idx[t] >= 0 is a record index into `inner`; -1 = empty tree
// (root = zero namespaces | SHA256("") for NMT, SHA256("") for RFC-6962);
// <= -2 is record -(idx + 2) of the leaf array `leaves`.  NMT roots are written
// as packed 90-B nodes (or 96-B records when records != 0); RFC-6962 roots as
// 32-B digests.
// out_stride: bytes between consecutive roots (0 = 90 / 96 / 32).
hipError_t launch_forest_roots(const uint8_t* leaves, const uint8_t* inner, const int64_t* root_idx,
                               long ntrees, int rfc, int records, uint8_t* out, long out_stride,
                               hipStream_t s);

// Push-order check over share vectors (ns = first 29 bytes of each share).
hipError_t launch_ns_order_check(const uint8_t* base, long nvec, long nper, long vec_stride, long elem_stride,
                                 int32_t* status, int bit, hipStream_t s);

// Packed 90-B nodes -> 96-B NMT records (the forest's record format).
hipError_t launch_node_to_rec(const uint8_t* nodes, long n, uint8_t* recs, hipStream_t s);

// Gather (row, depth, position) nodes of exported row trees as packed 90-B nodes.
hipError_t launch_node_gather(const uint8_t* nodes, int w, const uint32_t* req, long n, uint8_t* out,
                              hipStream_t s);

// Batched range proofs from the exported trees of resident squares
// (nmt_prove.hip).  Everything the host validated and laid out
// (prove_layout.hpp, share_proof_layout.hpp); the kernels check nothing.
// Square i's part of a region is at base + i * (bytes per square): the two
// exports of one square with strides 0 and no square in the requests, or the
// regions of a batch proof store.
struct ProveArgs {
  long n;                   // proofs
  int w, logw;              // leaves per tree (2k) and log2 of it
  int req_words;            // 8-B words per request: 1 (prove_pack_req) or 2 (that word, square)
  const int64_t* req;       // n requests
  const int64_t* node_off;  // n + 1 prefix sums: first output node of proof i
  const int64_t* leaf_off;  // n + 1 prefix sums: first output cell of proof i
  long n_nodes, n_leaves;   // node_off[n], leaf_off[n]
  const uint8_t* row_nodes; // dagpu_row_nodes_device stores (96-B records)
  const uint8_t* col_inner; // dagpu_col_nodes_device stores, null without axis-1 requests
  const uint8_t* eds;       // the squares, for the share gather
  const uint8_t* dah;       // the DAH trees of a batch proof store, for the merkle half
  long row_bytes, col_bytes, square_stride, dah_bytes;  // per square
  uint8_t* nodes_out;       // n_nodes packed 90-B nodes
  uint8_t* ns_out;          // n x 29 B or null
  uint8_t* shares_out;      // n_leaves x 512 B or null
  uint8_t* axis_roots_out;  // n x 90 B or null
  uint8_t* leaf_hash_out;   // n x 32 B or null
  uint8_t* aunts_out;       // n x log2(4k) x 32 B or null
};
hipError_t launch_prove_emit(const ProveArgs& a, hipStream_t s);
hipError_t launch_prove_namespaces(const ProveArgs& a, hipStream_t s);
hipError_t launch_prove_shares(const ProveArgs& a, hipStream_t s);
hipError_t launch_prove_sq_merkle(const ProveArgs& a, hipStream_t s);  // the three last outputs, from a.dah

// Batch proof store (proof_store.hip): every row-tree and column-tree node
// and the DAH tree of n squares, each level of all squares in one launch.
struct ProofStoreArgs {
  long n;             // squares
  int k, w, logw;     // w = 2k
  const uint8_t* eds; // square i at eds + i * square_stride
  long square_stride;
  uint8_t* store;
  long row_bytes, col_bytes, dah_bytes;  // per square
  long col_off, dah_off;                 // region starts
};
hipError_t launch_store_leaves(const ProofStoreArgs& a, hipStream_t s);
hipError_t launch_store_level(const ProofStoreArgs& a, int L, hipStream_t s);      // 1 <= L <= logw, rows and columns
hipError_t launch_store_dah_level(const ProofStoreArgs& a, int L, hipStream_t s);  // 0 <= L <= logw + 1

// Share commitments from squares resident in HBM (blob_commit.hip).  Every
// table was checked and laid out on the host (commit_layout.hpp); the kernels
// check nothing.
struct CommitArgs {
  const uint32_t* blob;       // nblobs x {square, first_share}
  const uint32_t* share_pre;  // nblobs + 1 prefix sums of share counts
  const uint32_t* sub_pre;    // nblobs + 1 prefix sums of subtree counts
  const uint32_t* sub;        // nsub x {blob, first leaf record, size}
  const uint32_t* work;       // nwork indexes of the subtrees of size >= 2
  uint32_t nblobs, nshares, nsub, nwork;
  uint32_t log2k;
  const uint8_t* squares;  // square i at squares + i * square_stride, rows row_pitch apart
  uint64_t square_stride, row_pitch;
  uint8_t* leaves;       // nshares 96-B records; even tree levels reuse them
  uint8_t* inner;        // nshares / 2 + 1 records: the odd tree levels
  uint8_t* dig0;         // nsub 32-B digests: RFC-6962 leaf level, then every second level
  uint8_t* dig1;         // the levels between
  uint8_t* commitments;  // nblobs x 32 B
  const uint8_t* expected;  // nblobs x 32 B or null
  int32_t* status;          // nblobs, zeroed before the subtree kernel
  int32_t* square_status;   // per square or null, zeroed before the commit kernel
};
hipError_t launch_commit_leaves(const CommitArgs& a, hipStream_t s);
hipError_t launch_commit_subtrees(const CommitArgs& a, hipStream_t s);
hipError_t launch_commit_roots(const CommitArgs& a, hipStream_t s);
// The counted forms: the tables are commit_plan.hip's image in device memory
// and the counts record {nblobs, nshares, nsub, nwork, ...} lies beside it, so
// `a` carries no table pointer and no count; the kernels stride over the items
// on a grid of min(capacity, grid_cap) workgroups.
struct CommitCounted {
  CommitArgs a;
  const uint32_t* tables;
  const uint32_t* counts;
};
hipError_t launch_commit_leaves_counted(const CommitCounted& c, uint64_t capacity, uint32_t grid_cap, hipStream_t s);
hipError_t launch_commit_subtrees_counted(const CommitCounted& c, uint64_t capacity, uint32_t grid_cap, hipStream_t s);
hipError_t launch_commit_roots_counted(const CommitCounted& c, uint64_t capacity, uint32_t grid_cap, hipStream_t s);

// Namespace search over the row trees of one square (nmt_namespace.hip;
// arithmetic in ns_find.hpp).  One lane per (query, row).
struct NsFindArgs {
  long n_q;                  // queries
  int w;                     // leaves per row tree (2k)
  const uint8_t* queries;    // n_q namespaces, zero padded to 32 B, 16-B aligned
  const uint8_t* row_nodes;  // dagpu_row_nodes_device store (96-B records)
  int32_t* ranges;           // n_q x w x {kind, start, end}
};
hipError_t launch_ns_find(const NsFindArgs& a, hipStream_t s);
// Level-0 records rec_index[0 .. n) as packed 90-B nodes, the leaf hashes of
// absence proofs; indexes count 96-B records from `base`, a row store or the
// row region of a batch proof store.
hipError_t launch_ns_leaf_nodes(const uint8_t* base, const int64_t* rec_index, long n, uint8_t* out, hipStream_t s);

// The same search across the squares of a batch proof store, with the proofs
// counted, ordered and laid out on the device (nmt_namespace.hip; arithmetic
// and workspace carve in ns_squares_layout.hpp).  One lane per (query, square,
// row); every pointer but queries / store points into the workspace.
struct NsSqArgs {
  long n_q, n_sq;
  int w, logw;              // leaves per row tree (2k) and log2 of it
  long lanes, pairs;        // n_q * n_sq * w, n_q * n_sq
  long blocks, chunks;      // blocks of 256 lanes, chunks of 256 blocks
  const uint8_t* queries;   // n_q namespaces, zero padded to 32 B, 16-B aligned
  const uint8_t* store;     // the batch proof store: square i's rows at i * row_bytes
  long row_bytes;
  uint32_t* words;          // lanes packed ranges (ns_sq_pack)
  int64_t* bsum;            // blocks x 4 sums
  int64_t* csum;            // chunks x 4 sums
  int64_t* totals;          // 4: proofs, absence proofs, proof nodes, proven cells
  int32_t* per;             // pairs proof counts, or null
  // written by the scatter, for ProveArgs (two-word requests) and the host
  int64_t* req;             // proofs x {prove_pack_req word, square}
  int64_t* node_off;        // proofs + 1
  int64_t* leaf_off;        // proofs + 1
  int64_t* abs_rec;         // absence proofs: level-0 record index in the row region
  uint32_t* hits;           // proofs x {lane, packed range}
};
// find, block sums, the two scan levels and (with a.per) the per-pair counts
hipError_t launch_ns_sq_search(const NsSqArgs& a, hipStream_t s);
// after the host has compared a.totals with the capacities
hipError_t launch_ns_sq_scatter(const NsSqArgs& a, hipStream_t s);

// Host-side level plan of one forest.  Leaves (level 0) are either packed tree
// after tree (ragged: counts[t] leaves each) or uniform with (tstride,
// lstride) addressing inside a caller-owned leaf array.  Levels >= 1 are packed
// tree-major, one after another, in a single record buffer.
struct ForestPlan {
  long ntrees = 0;
  bool uniform = true;
  long per0 = 0;                 // uniform leaf count
  long tstride0 = 0, lstride0 = 1;
  std::vector<long> counts0;     // ragged leaf counts
  int nlevels = 0;               // inner levels (level 1..nlevels)
  std::vector<long> total;       // total[L] nodes at level L (L >= 1)
  std::vector<long> base;        // base[L] record offset of level L in the inner buffer
  std::vector<long> per;         // uniform: nodes per tree at level L
  std::vector<std::vector<int64_t>> off;  // ragged: off[L] (ntrees + 1 prefix sums), L >= 0
  // root_idx per tree in the launch_forest_roots encoding
  std::vector<int64_t> root_idx;
  long inner_records = 0;        // records needed for levels >= 1
  // device metadata image: ragged offset arrays then root_idx (int64)
  std::vector<int64_t> meta;
  std::vector<long> meta_off;    // meta_off[L]: start of off[L] in meta (ragged)
  long meta_root = 0;            // start of root_idx in meta
  void finalize();

  static ForestPlan uniform_plan(long ntrees, long leaves, long tstride, long lstride);
  static ForestPlan ragged_plan(const std::vector<long>& counts);
};

// Enqueue every inner level and the roots of plan `p` on stream s.
//   d_leaves  level-0 records (rec = 96 B NMT / 32 B RFC-6962)
//   d_inner   p.inner_records records
//   d_meta    p.meta.size() int64 (ragged plans: uploaded here, keep `p` alive
//             until the stream has passed this point; uniform plans upload
//             nothing and need neither)
//   d_status  per-tree status (check_order), may be null otherwise
//   d_roots   ntrees roots (90 B packed / 96 B records / 32 B digests)
hipError_t forest_enqueue(const ForestPlan& p, const uint8_t* d_leaves, uint8_t* d_inner, int64_t* d_meta,
                          int ignore_max, int check_order, int rfc, int32_t* d_status, uint8_t* d_roots,
                          int records, long roots_stride, hipStream_t s);

// Two forests hashed level by level in shared launches (level L of both in
// one grid): the column trees and the row subtrees of a split slab.
struct ForestJob {
  const ForestPlan* p;
  const uint8_t* d_leaves;
  uint8_t* d_inner;
  int64_t* d_meta;
  int ignore_max, check_order, rfc;
  int32_t* d_status;
  uint8_t* d_roots;
  int records;
  long roots_stride;
  int status_shared = 0;  // ForestLevelArgs::status_shared
};
hipError_t forest_enqueue_pair(const ForestJob& x, const ForestJob& y, hipStream_t s);

}  // namespace dagpu
