// square_plan.hpp -- the parse and layout arithmetic of square.Construct
// (pkg/square/builder.go, pkg/blob/blob.go, pkg/inclusion) in one copy for the
// host (square.cpp: SquareBuilder) and the device planner (square_plan.hip,
// dagpu_square_plan_device), and the planner itself: sp_classify_tx (one lane
// per tx) and sp_plan_block (one workgroup per block), written once over an
// execution policy X.  The kernels instantiate them with 256 lanes, wave
// shuffles and barriers; dagpu_square_plan_emulate_host with a policy that
// runs the 256 lanes of every phase as a loop, so the CPU tests run the
// arithmetic, the chunking and the sorting network the GPU runs.  Plain
// arithmetic only (no HIP include); every function is marked for both sides
// when hipcc compiles it.
//
// sp_plan_block, per block (phases are separated by barriers; what one phase
// hands to the next lies in SpShared or in the workspace, never in a lane):
//   scan     over the txs in chunks of kSpLanes: the running sums that
//            Builder.AppendTx / AppendBlobTx keep (bytes of the two delimited
//            unit streams, blob shares + max padding), the first tx at which
//            Construct stops (min over status words), and where each normal
//            tx's delimiter, segments and literal go
//   fill     the blob records (second parse of the blob txs), at the scanned
//            positions: (pfb ordinal, blob index) order
//   sort     bitonic network over the blob indexes in LDS by (namespace,
//            position): a total order, so the result is std::stable_sort's
//   layout   one lane walks NextShareIndex over the sorted blobs (share
//            counts and subtree widths staged in LDS), with Export's checks
//   pfb      actual IndexWrapper sizes from the scattered share indexes; scan
//            of stream positions, segments and literals; WriteSquare's checks
//   emit     the plan of square_write.hpp, byte for byte dagpu_square_plan's
#pragma once
#include <stdint.h>
#include <string.h>

#include "square_write.hpp"

namespace dagpu {

constexpr uint32_t kSpLanes = 256;          // lanes of a block's workgroup = txs per scan chunk
constexpr uint32_t kSpMaxWidth = 128;       // max_square_size the planner takes
constexpr uint32_t kSpMaxBlobs = 128 * 128; // blob indexes of one block in LDS
constexpr uint32_t kSpMaxTxs = 1u << 24;    // txs of one block: the status word keeps the index above 8 bits
constexpr uint32_t kSpNsId = 28;
constexpr uint32_t kSpWorstIndex = 128u * 128u;  // AppendBlobTx: every share index SquareSizeUpperBound^2

// status word: kind | index << 8
enum : uint32_t {
  kSpOk = 0,
  kSpNoSpaceTx = 1,      // "not enough space to append tx at index i"
  kSpNoSpaceBlobTx = 2,  // "not enough space to append blob tx at index i"
  kSpTxAfterBlobTx = 3,  // "normal tx at index i can not be appended after blob tx"
  kSpLayout = 4,         // any error of SquareBuilder::layout(); index = sorted blob, or 0
  kSpTooManyBlobs = 5,   // more than max_square_size^2 blobs
  kSpWidth = 6,          // dagpu_square_construct_device: the width (index) is not the call's
  kSpArena = 7,          // the plan arena is smaller than the documented bound
};

// ---- varints ----------------------------------------------------------------
DAGPU_SQ_HD inline uint32_t uvarint_len(uint64_t v) {
  uint32_t n = 1;
  while (v >= 0x80) {
    v >>= 7;
    n++;
  }
  return n;
}
DAGPU_SQ_HD inline uint32_t put_uvarint(uint8_t* out, uint64_t v) {
  uint32_t n = 0;
  while (v >= 0x80) {
    out[n++] = (uint8_t)(v | 0x80);
    v >>= 7;
  }
  out[n++] = (uint8_t)v;
  return n;
}
// false: unexpected end of the buffer, or a varint past 64 bits
DAGPU_SQ_HD inline bool read_varint(const uint8_t* b, uint32_t n, uint32_t& i, uint64_t& v) {
  v = 0;
  for (unsigned s = 0;; s += 7) {
    if (i >= n || s >= 64) return false;
    const uint8_t c = b[i++];
    v |= (uint64_t)(c & 0x7F) << s;
    if (c < 0x80) return true;
  }
}

// ---- gogoproto field walk as a cursor ---------------------------------------
// One step over b[0, n): 1 and the field (number, wire type, varint value or
// the span [off, off + len) of a length-delimited field), 0 at the end, -1 for
// a malformed buffer: field number 0, wire types 3, 4, 6, 7, a bad varint or a
// field running past n.  Wire types 1 and 5 are skipped over.  No byte at or
// past n is read.
struct SpField {
  uint64_t num, v;
  uint32_t wt, off, len;
};
DAGPU_SQ_HD inline int sp_next_field(const uint8_t* b, uint32_t n, uint32_t& i, SpField& f) {
  if (i >= n) return 0;
  uint64_t key;
  if (!read_varint(b, n, i, key)) return -1;
  f.num = key >> 3;
  f.wt = (uint32_t)(key & 7);
  f.v = 0;
  f.off = f.len = 0;
  if (f.num == 0) return -1;
  switch (f.wt) {
    case 0:
      if (!read_varint(b, n, i, f.v)) return -1;
      break;
    case 1:
      if (n - i < 8) return -1;
      i += 8;
      break;
    case 2: {
      uint64_t len;
      if (!read_varint(b, n, i, len) || len > n - i) return -1;
      f.off = i;
      f.len = (uint32_t)len;
      i += (uint32_t)len;
      break;
    }
    case 5:
      if (n - i < 4) return -1;
      i += 4;
      break;
    default:
      return -1;
  }
  return 1;
}

// ---- shares -----------------------------------------------------------------
DAGPU_SQ_HD inline uint64_t round_up_pow2(uint64_t v) {
  uint64_t r = 1;
  while (r < v) r <<= 1;
  return r;
}
// inclusion.BlobMinSquareSize: RoundUpPowerOfTwo(ceil(sqrt(n))) = the smallest
// power of two r with r * r >= n (an integer r is >= ceil(sqrt(n)) iff
// r * r >= n); tests/host/square_plan_check.cpp compares it with the double form
DAGPU_SQ_HD inline uint64_t blob_min_square_size(uint64_t share_count) {
  uint64_t r = 1;
  while (r * r < share_count) r <<= 1;
  return r;
}
DAGPU_SQ_HD inline uint64_t subtree_width_u(uint64_t share_count, uint64_t threshold) {
  uint64_t s = share_count / threshold + (share_count % threshold ? 1 : 0);
  s = round_up_pow2(s);
  const uint64_t m = blob_min_square_size(share_count);
  return s < m ? s : m;
}
DAGPU_SQ_HD inline uint64_t sparse_shares_needed(uint64_t len) {
  if (len == 0) return 0;
  if (len < kSqFirstSparse) return 1;
  return 1 + (len - kSqFirstSparse + kSqContSparse - 1) / kSqContSparse;
}
// shares.CompactSharesNeeded: compact shares a unit stream of len bytes fills
DAGPU_SQ_HD inline uint64_t compact_shares_needed(uint64_t len) {
  if (len == 0) return 0;
  if (len <= kSqFirstCompact) return 1;
  return 1 + (len - kSqFirstCompact + kSqContCompact - 1) / kSqContCompact;
}
// inclusion.NextShareIndex: the next multiple of the blob's subtree width
DAGPU_SQ_HD inline uint64_t next_share_index(uint64_t cursor, uint64_t width) {
  return cursor % width == 0 ? cursor : (cursor / width + 1) * width;
}
// namespace.From: 0 = valid, 1 = unsupported version, 2 = a version-0 ID
// without its 18 leading zeros.  byte(i): byte i of the 29-byte namespace.
template <class B>
DAGPU_SQ_HD inline int namespace_fault_of(B&& byte) {
  const uint8_t v = byte(0);
  if (v != 0 && v != 255) return 1;
  if (v == 0)
    for (uint32_t i = 1; i <= 18; i++)
      if (byte(i)) return 2;
  return 0;
}
DAGPU_SQ_HD inline int namespace_fault(const uint8_t* ns) {
  return namespace_fault_of([ns](uint32_t i) { return ns[i]; });
}

// ---- tmproto.IndexWrapper sizes ---------------------------------------------
// tx = 1, share_indexes = 2 (packed), type_id = 3 "INDX".  packed: the bytes of
// the share indexes' varints; n_idx = 0: no field 2.
DAGPU_SQ_HD inline uint64_t index_wrapper_size_packed(uint64_t tx_len, uint64_t n_idx, uint64_t packed) {
  uint64_t s = 6;  // type_id field
  if (tx_len) s += 1 + uvarint_len(tx_len) + tx_len;
  if (n_idx) s += 1 + uvarint_len(packed) + packed;
  return s;
}
DAGPU_SQ_HD inline uint64_t index_wrapper_size(uint64_t tx_len, uint64_t n_idx, uint32_t each) {
  return index_wrapper_size_packed(tx_len, n_idx, n_idx * uvarint_len(each));
}
DAGPU_SQ_HD inline uint64_t index_wrapper_size(uint64_t tx_len, const uint32_t* idx, uint64_t n_idx) {
  uint64_t packed = 0;
  for (uint64_t i = 0; i < n_idx; i++) packed += uvarint_len(idx[i]);
  return index_wrapper_size_packed(tx_len, n_idx, packed);
}

// ---- blob.UnmarshalBlobTx ---------------------------------------------------
// One blob of a BlobTx; offsets from the start of the tx.  ns_len = 0 and
// data_len = 0 when the field is absent.
struct SpBlobFields {
  uint32_t ns_off, ns_len, data_off, data_len, share_version, ns_version;
};
struct SpTxInfo {
  uint32_t is_blob_tx;  // decodes, type_id "BLOB", >= 1 blob, every namespace ID 28 bytes
  uint32_t inner_off, inner_len;
  uint32_t nblob;
  uint64_t cost;  // sum over the blobs of shares + max padding (AppendBlobTx), when threshold != 0
};
// Count mode (out == nullptr): the verdict, the inner tx and the blob count.
// Fill mode: also one record per blob, record j at (uint8_t*)out + j * stride,
// for the first out_cap blobs.  Last field 1, last field 3 and inside a blob
// the last of each field win; share and namespace version are cut to 32 bits
// as the reference's uint32 fields are.  Reads tx[0, n) only.
DAGPU_SQ_HD inline SpTxInfo sp_unmarshal_blob_tx(const uint8_t* tx, uint32_t n, uint32_t threshold,
                                                 SpBlobFields* out, uint32_t out_cap, uint32_t stride) {
  SpTxInfo r;
  r.is_blob_tx = r.inner_off = r.inner_len = r.nblob = 0;
  r.cost = 0;
  uint32_t i = 0, type_off = 0, type_len = 0;
  bool ids_ok = true;
  SpField f;
  for (;;) {
    const int st = sp_next_field(tx, n, i, f);
    if (st < 0) return r;
    if (st == 0) break;
    if (f.num == 1) {
      if (f.wt != 2) return r;
      r.inner_off = f.off;
      r.inner_len = f.len;
    } else if (f.num == 2) {
      if (f.wt != 2) return r;
      SpBlobFields b;
      b.ns_off = b.ns_len = b.data_off = b.data_len = b.share_version = b.ns_version = 0;
      const uint8_t* m = tx + f.off;
      uint32_t j = 0;
      SpField g;
      for (;;) {
        const int s2 = sp_next_field(m, f.len, j, g);
        if (s2 < 0) return r;
        if (s2 == 0) break;
        if (g.num == 1) {
          if (g.wt != 2) return r;
          b.ns_off = f.off + g.off;
          b.ns_len = g.len;
        } else if (g.num == 2) {
          if (g.wt != 2) return r;
          b.data_off = f.off + g.off;
          b.data_len = g.len;
        } else if (g.num == 3) {
          if (g.wt != 0) return r;
          b.share_version = (uint32_t)g.v;
        } else if (g.num == 4) {
          if (g.wt != 0) return r;
          b.ns_version = (uint32_t)g.v;
        }
      }
      if (b.ns_len != kSpNsId) ids_ok = false;
      if (threshold) {
        const uint64_t shares = sparse_shares_needed(b.data_len);
        r.cost += shares + subtree_width_u(shares, threshold) - 1;
      }
      if (out && r.nblob < out_cap) *(SpBlobFields*)((uint8_t*)out + (size_t)r.nblob * stride) = b;
      r.nblob++;
    } else if (f.num == 3) {
      if (f.wt != 2) return r;
      type_off = f.off;
      type_len = f.len;
    }
  }
  if (type_len != 4 || tx[type_off] != 'B' || tx[type_off + 1] != 'L' || tx[type_off + 2] != 'O' ||
      tx[type_off + 3] != 'B' || r.nblob == 0 || !ids_ok)
    return r;
  r.is_blob_tx = 1;
  return r;
}

// ---- the device planner's tables ----------------------------------------------
struct SpBlockIn {   // per block, from the host
  uint64_t src_off;  // of the block's packed txs inside src
  uint64_t blob_at;  // the block's first record in the blob record array
  uint32_t src_len, tx_base, ntx, pad;
};
struct SpTxIn {  // per tx, from the host
  uint32_t off, len, blk, pad;
};
struct SpTxCls {  // per tx, from sp_classify_tx; blob_at and pfb_ord from the block's scan
  uint32_t is_blob_tx, inner_off, inner_len, nblob;
  uint32_t cost, iw_worst, blob_at, pfb_ord;
};
struct SpTxPos {  // where a unit starts in its stream, its first segment, its first literal byte
  uint32_t pos, seg, lit, pad;
};
struct SpBlobRec {
  uint64_t key[4];  // the 29-byte namespace as big-endian words, zero padded
  // fill mode's SpBlobFields; then ns_off / ns_len become pfb ordinal / blob index
  uint32_t pfb_ord, blob_idx, data_off, data_len, share_version, ns_version;
  uint32_t start, shares;
};
static_assert(sizeof(SpBlobRec) == 64 && sizeof(SpTxCls) == 32 && sizeof(SpBlockIn) == 32, "planner tables");
struct SpRecord {     // per block, the planner's result
  uint64_t plan_off;  // of the plan inside the arena, 16-B aligned
  uint64_t src_off;   // of the block's packed txs inside src
  uint32_t plan_bytes, k, status, nblob;
};
struct SpArgs {
  const uint8_t* src;
  const SpBlockIn* blk;
  const SpTxIn* tx;
  SpTxCls* cls;
  SpTxPos* pos;
  SpBlobRec* blobs;
  uint16_t* sorted;  // kSpMaxBlobs per block: the sorted blob order
  uint8_t* arena;
  uint64_t arena_cap;
  unsigned long long* cursor;  // bytes of the arena handed out
  unsigned long long* clocks;  // DAGPU_PLAN_CLOCKS builds: 8 per block, X::clock() at the start and after each phase
  SpRecord* rec;
  uint32_t* status;
  uint32_t n, max_square_size, threshold;
};

// Documented bounds (include/dagpu.h): bytes of one block's plan and of the
// workspace.  Segments: at most 2 per tx, one more for the first PFB, and the
// two end pairs; units: 1 per tx; blobs: max_square_size^2; literals: a tx
// delimiter is at most 5 bytes, a PFB's head uvarint(size) + 0x0a +
// uvarint(inner length) at most 11, its tail 0x12 + uvarint(packed) at most 4,
// the type_id field 6, and at most 3 bytes per share index; 16 bytes of
// alignment behind each of the 6 tables.
DAGPU_SQ_HD inline uint64_t sp_plan_bound(uint64_t ntx, uint32_t max_square_size) {
  const uint64_t blobs = (uint64_t)max_square_size * max_square_size;
  return sizeof(SqHdr) + (2 * ntx + 3) * 8 + ntx * 4 + blobs * kSqBlobWords * 4 + ntx * 21 + blobs * 3 + 6 * 16;
}
DAGPU_SQ_HD inline uint64_t sp_up16(uint64_t v) { return (v + 15) & ~(uint64_t)15; }
// A measurement build (-DDAGPU_PLAN_CLOCKS, tools/build_variant.sh) has every
// block's workgroup leave a wall clock per phase in 64 more bytes per block at
// the workspace's end; the product library has neither the bytes nor the stores.
#if defined(DAGPU_PLAN_CLOCKS)
constexpr bool kSpClocks = true;
#else
constexpr bool kSpClocks = false;
#endif
// workspace: cursor | SpBlockIn[n] | SpTxIn[ntx] | SpTxCls[ntx] | SpTxPos[ntx] | sorted | SpBlobRec [| clocks]
struct SpCarve {
  uint64_t blk, tx, cls, pos, sorted, blobs, clocks, total;
};
DAGPU_SQ_HD inline SpCarve sp_carve(uint64_t n, uint64_t ntx, uint32_t max_square_size) {
  const uint64_t blobs = (uint64_t)max_square_size * max_square_size;
  SpCarve c;
  c.blk = 16;
  c.tx = c.blk + n * sizeof(SpBlockIn);
  c.cls = c.tx + ntx * sizeof(SpTxIn);
  c.pos = c.cls + ntx * sizeof(SpTxCls);
  c.sorted = c.pos + ntx * sizeof(SpTxPos);
  c.blobs = sp_up16(c.sorted + n * kSpMaxBlobs * 2);
  c.clocks = c.blobs + n * blobs * sizeof(SpBlobRec);
  c.total = c.clocks + (kSpClocks ? n * 64 : 0);
  return c;
}

// ---- classify: one lane per tx ----------------------------------------------
DAGPU_SQ_HD inline void sp_classify_tx(const SpArgs& a, uint64_t g) {
  const SpTxIn t = a.tx[g];
  const uint8_t* p = a.src + a.blk[t.blk].src_off + t.off;
  const SpTxInfo r = sp_unmarshal_blob_tx(p, t.len, a.threshold, nullptr, 0, 0);
  SpTxCls c;
  c.is_blob_tx = r.is_blob_tx;
  c.inner_off = r.inner_off;
  c.inner_len = r.inner_len;
  c.nblob = r.nblob;
  c.cost = (uint32_t)r.cost;
  c.iw_worst = (uint32_t)index_wrapper_size(r.inner_len, r.nblob, kSpWorstIndex);
  c.blob_at = c.pfb_ord = 0;
  a.cls[g] = c;
}

// ---- one block ----------------------------------------------------------------
constexpr uint32_t kSpScanVals = 7;
struct SpShared {
  uint16_t x[kSpMaxBlobs];  // sort: blob indexes; layout: share counts, then first shares
  uint8_t y[kSpMaxBlobs];   // layout: log2(subtree width) | namespace fault << 3 | blob fault << 4
  uint32_t v[kSpScanVals][kSpLanes];
  uint32_t wave[kSpScanVals][kSpLanes / 64];
  uint32_t carry[kSpScanVals];
  uint32_t fail;  // the lowest status word of a failing tx
  uint32_t status, k, n_normal, nrs, end_of_last;
  uint32_t lit0;
  uint64_t plan_off;
  SqHdr hdr;
};

// the values the scan sums for tx i
DAGPU_SQ_HD inline void sp_tx_vals(const SpArgs& a, const SpBlockIn& b, uint32_t i, uint32_t* v) {
  const SpTxCls c = a.cls[b.tx_base + i];
  const uint32_t len = a.tx[b.tx_base + i].len;
  for (uint32_t j = 0; j < kSpScanVals; j++) v[j] = 0;
  if (c.is_blob_tx) {
    v[1] = uvarint_len(c.iw_worst) + c.iw_worst;
    v[2] = c.cost;
    v[3] = c.nblob;
    v[4] = 1;
  } else {
    v[0] = uvarint_len(len) + len;
    // literals written back to back are one segment: a delimiter opens one
    // only behind a tx with bytes
    v[5] = ((i == 0 || a.tx[b.tx_base + i - 1].len) ? 1 : 0) + (len ? 1 : 0);
    v[6] = uvarint_len(len);
  }
}
// the same for PFB p (tx i), from the share indexes the layout scattered
struct SpPfb {
  uint32_t packed, iw, head, tail;
};
DAGPU_SQ_HD inline SpPfb sp_pfb(const SpTxCls& c, const SpBlobRec* blobs) {
  SpPfb r;
  r.packed = 0;
  for (uint32_t j = 0; j < c.nblob; j++) r.packed += uvarint_len(blobs[c.blob_at + j].start);
  r.iw = (uint32_t)index_wrapper_size_packed(c.inner_len, c.nblob, r.packed);
  r.head = uvarint_len(r.iw) + (c.inner_len ? 1 + uvarint_len(c.inner_len) : 0);
  r.tail = 1 + uvarint_len(r.packed) + r.packed + 6;
  return r;
}
DAGPU_SQ_HD inline uint64_t sp_bswap64(uint64_t v) {
  v = (v >> 32) | (v << 32);
  v = ((v & 0xFFFF0000FFFF0000ull) >> 16) | ((v & 0x0000FFFF0000FFFFull) << 16);
  return ((v & 0xFF00FF00FF00FF00ull) >> 8) | ((v & 0x00FF00FF00FF00FFull) << 8);
}
// (namespace, position) order over blob indexes; 0xFFFF pads the network and sorts last
DAGPU_SQ_HD inline bool sp_blob_less(const SpBlobRec* blobs, uint32_t p, uint32_t q) {
  if (p == 0xFFFF) return false;
  if (q == 0xFFFF) return true;
  for (int w = 0; w < 4; w++) {
    const uint64_t x = blobs[p].key[w], y = blobs[q].key[w];
    if (x != y) return x < y;
  }
  return p < q;
}

// X: T lanes; each(f) runs f(lane) on every lane, then a barrier; one(f) runs
// f() on lane 0, then a barrier; scan(v, wave) turns the kSpScanVals rows of v
// into inclusive sums over the lanes; take(cursor, bytes) hands out arena bytes;
// clock() is a wall clock for the phase times (0 on the host).
template <class X>
DAGPU_SQ_HD inline void sp_plan_block(X& x, SpShared& s, const SpArgs& a, uint32_t blk) {
  constexpr uint32_t T = kSpLanes;
  const SpBlockIn b = a.blk[blk];
  const uint32_t cap = a.max_square_size * a.max_square_size;
  const uint8_t* src = a.src + b.src_off;
  SpBlobRec* blobs = a.blobs + b.blob_at;
  uint16_t* sorted = a.sorted + (uint64_t)blk * kSpMaxBlobs;

  // measurement builds only.  phase i is over: clocks 1 scan, 2 fill, 3 sort, 4 layout, 5 pfb, 6 emit (0 where a phase did not run)
  auto mark = [&](uint32_t i) {
    if constexpr (kSpClocks) x.one([&] { a.clocks[(uint64_t)blk * 8 + i] = x.clock(); });
  };

  // ---- scan ----
  x.one([&] {
    if constexpr (kSpClocks) {
      for (uint32_t j = 1; j < 8; j++) a.clocks[(uint64_t)blk * 8 + j] = 0;
      a.clocks[(uint64_t)blk * 8] = x.clock();
    }
    for (uint32_t j = 0; j < kSpScanVals; j++) s.carry[j] = 0;
    s.fail = 0xFFFFFFFFu;
    s.status = 0;
  });
  for (uint32_t base = 0; base < b.ntx; base += T) {
    x.each([&](uint32_t t) {
      uint32_t v[kSpScanVals];
      for (uint32_t j = 0; j < kSpScanVals; j++) v[j] = 0;
      if (base + t < b.ntx) sp_tx_vals(a, b, base + t, v);
      for (uint32_t j = 0; j < kSpScanVals; j++) s.v[j][t] = v[j];
    });
    x.scan(s.v, s.wave);
    x.each([&](uint32_t t) {
      const uint32_t i = base + t;
      if (i >= b.ntx) return;
      uint32_t own[kSpScanVals], inc[kSpScanVals];
      sp_tx_vals(a, b, i, own);
      for (uint32_t j = 0; j < kSpScanVals; j++) inc[j] = s.carry[j] + s.v[j][t];
      const bool blob = own[4] != 0;
      // current_ after tx i, had every tx up to i been appended
      const uint64_t cur = compact_shares_needed(inc[0]) + compact_shares_needed(inc[1]) + inc[2];
      uint32_t kind = 0;
      if (!blob && inc[4] != 0) kind = kSpTxAfterBlobTx;
      else if (cur > cap) kind = blob ? kSpNoSpaceBlobTx : kSpNoSpaceTx;
      if (kind) x.lowest(&s.fail, kind | (i << 8));
      if (blob) {
        a.cls[b.tx_base + i].blob_at = inc[3] - own[3];
        a.cls[b.tx_base + i].pfb_ord = inc[4] - 1;
      } else {
        SpTxPos p;
        p.pos = inc[0] - own[0];
        p.seg = inc[5] - own[5];
        p.lit = inc[6] - own[6];
        p.pad = 0;
        a.pos[b.tx_base + i] = p;
      }
    });
    x.one([&] {
      for (uint32_t j = 0; j < kSpScanVals; j++) s.carry[j] += s.v[j][T - 1];
    });
  }
  // carry: 0 tx stream bytes, 1 worst-case PFB stream bytes, 2 blob shares +
  // max padding, 3 blobs, 4 PFBs, 5 tx segments, 6 tx literal bytes
  x.one([&] {
    const uint64_t cur = compact_shares_needed(s.carry[0]) + compact_shares_needed(s.carry[1]) + s.carry[2];
    s.k = b.ntx == 0 ? 1 : (uint32_t)blob_min_square_size(cur);
    s.n_normal = b.ntx - s.carry[4];
    s.lit0 = s.carry[6];
    if (s.fail != 0xFFFFFFFFu) s.status = s.fail;
    else if (s.carry[3] > cap) s.status = kSpTooManyBlobs;
    s.nrs = s.end_of_last = (uint32_t)(compact_shares_needed(s.carry[0]) + compact_shares_needed(s.carry[1]));
  });
  const uint32_t nblob = s.status ? 0 : s.carry[3], npfb = s.status ? 0 : s.carry[4];
  const uint32_t n_normal = s.n_normal, seq0_len = s.carry[0], nseg0 = s.carry[5];
  const uint32_t worst_pfb_shares = (uint32_t)compact_shares_needed(s.carry[1]);

  mark(1);
  if (!s.status) {
    // ---- fill: blob records in (pfb ordinal, blob index) order ----
    x.each([&](uint32_t t) {
      for (uint32_t p = t; p < npfb; p += T) {
        const SpTxIn tx = a.tx[b.tx_base + n_normal + p];
        const SpTxCls c = a.cls[b.tx_base + n_normal + p];
        SpBlobRec* out = blobs + c.blob_at;
        sp_unmarshal_blob_tx(src + tx.off, tx.len, 0, (SpBlobFields*)&out->pfb_ord, c.nblob, sizeof(SpBlobRec));
        for (uint32_t j = 0; j < c.nblob; j++) {
          SpBlobRec& r = out[j];
          const uint8_t* id = src + tx.off + r.pfb_ord;  // fill mode's ns_off; ns_len is 28
          const uint8_t version = (uint8_t)r.ns_version;
          for (uint32_t w = 0; w < 4; w++) {
            uint64_t key = 0;
            for (uint32_t q = 8 * w; q < 8 * w + 8; q++)
              key = key << 8 | (q == 0 ? version : q <= kSpNsId ? id[q - 1] : (uint8_t)0);
            r.key[w] = key;
          }
          r.pfb_ord = p;
          r.blob_idx = j;
          r.data_off += tx.off;
          r.shares = (uint32_t)sparse_shares_needed(r.data_len);
          r.start = 0;
        }
      }
    });
    mark(2);
    // ---- sort ----
    uint32_t npad = 1;
    while (npad < nblob) npad <<= 1;
    x.each([&](uint32_t t) {
      for (uint32_t i = t; i < npad; i += T) s.x[i] = i < nblob ? (uint16_t)i : (uint16_t)0xFFFF;
    });
    for (uint32_t kk = 2; kk <= npad; kk <<= 1)
      for (uint32_t j = kk >> 1; j > 0; j >>= 1)
        x.each([&](uint32_t t) {
          for (uint32_t e = t; e < npad / 2; e += T) {
            const uint32_t lo = ((e & ~(j - 1)) << 1) | (e & (j - 1)), hi = lo | j;
            const bool up = (lo & kk) == 0;
            const uint16_t p = s.x[lo], q = s.x[hi];
            if (sp_blob_less(blobs, q, p) == up) {
              s.x[lo] = q;
              s.x[hi] = p;
            }
          }
        });
    mark(3);
    // ---- layout ----
    x.each([&](uint32_t t) {
      for (uint32_t i = t; i < nblob; i += T) sorted[i] = s.x[i];
    });
    x.each([&](uint32_t t) {
      for (uint32_t i = t; i < nblob; i += T) {
        const SpBlobRec& r = blobs[sorted[i]];
        const int ns_fault =
            namespace_fault_of([&r](uint32_t i) { return (uint8_t)(r.key[i >> 3] >> (56 - 8 * (i & 7))); });
        uint32_t lg = 0;
        const uint64_t w = subtree_width_u(r.shares, a.threshold);
        while ((1ull << lg) < w) lg++;
        const bool blob_fault = r.share_version != 0 || r.ns_version > 255 || r.data_len == 0;
        s.x[i] = (uint16_t)r.shares;  // <= max_square_size^2: the block passed the append loop
        s.y[i] = (uint8_t)(lg | (ns_fault ? 8 : 0) | (blob_fault ? 16 : 0));
      }
    });
    x.one([&] {
      uint32_t cursor = s.nrs, end = s.nrs;
      bool prev_ns_fault = false;
      for (uint32_t i = 0; i < nblob; i++) {
        const uint32_t f = s.y[i], w = 1u << (f & 7);
        cursor = (uint32_t)next_share_index(cursor, w);
        if (i == 0) s.nrs = cursor;
        const uint32_t padding = cursor - end;
        // Export's checks in its order: the padding, the padding shares'
        // namespace (the previous blob's), Blob.ValidateBasic, the share version
        if (padding > w - 1 || (i > 0 && padding > 0 && prev_ns_fault) || (f & 16)) {
          s.status = kSpLayout | (i << 8);
          break;
        }
        const uint32_t shares = s.x[i];
        s.x[i] = (uint16_t)cursor;
        cursor += shares;
        end = cursor;
        prev_ns_fault = (f & 8) != 0;
      }
      s.end_of_last = end;
    });
    mark(4);
  }
  if (!s.status) {
    x.each([&](uint32_t t) {
      for (uint32_t i = t; i < nblob; i += T) blobs[sorted[i]].start = s.x[i];
    });
    // ---- pfb stream: rows 0 stream bytes, 1 segments, 2 literal bytes ----
    x.one([&] {
      for (uint32_t j = 0; j < kSpScanVals; j++) s.carry[j] = 0;
    });
    for (uint32_t base = 0; base < npfb; base += T) {
      x.each([&](uint32_t t) {
        for (uint32_t j = 0; j < kSpScanVals; j++) s.v[j][t] = 0;
        const uint32_t p = base + t;
        if (p >= npfb) return;
        const SpTxCls c = a.cls[b.tx_base + n_normal + p];
        const SpPfb f = sp_pfb(c, blobs);
        s.v[0][t] = uvarint_len(f.iw) + f.iw;
        s.v[1][t] = (p == 0 ? 1 : 0) + (c.inner_len ? 2 : 0);
        s.v[2][t] = f.head + f.tail;
      });
      x.scan(s.v, s.wave);
      x.each([&](uint32_t t) {
        const uint32_t p = base + t;
        if (p >= npfb) return;
        const SpTxCls c = a.cls[b.tx_base + n_normal + p];
        const SpPfb f = sp_pfb(c, blobs);
        SpTxPos o;
        o.pos = s.carry[0] + s.v[0][t] - (uvarint_len(f.iw) + f.iw);
        o.seg = s.carry[1] + s.v[1][t] - ((p == 0 ? 1 : 0) + (c.inner_len ? 2 : 0));
        o.lit = s.lit0 + s.carry[2] + s.v[2][t] - (f.head + f.tail);
        o.pad = 0;
        a.pos[b.tx_base + n_normal + p] = o;
      });
      x.one([&] {
        for (uint32_t j = 0; j < 3; j++) s.carry[j] += s.v[j][T - 1];
      });
    }
    // ---- WriteSquare's checks, the header, the plan's place ----
    x.one([&] {
      const uint32_t seq1_len = s.carry[0], nseg1 = s.carry[1], lit_bytes = s.lit0 + s.carry[2];
      const uint32_t pfb_count = (uint32_t)compact_shares_needed(seq1_len);
      const uint32_t pfb_start = (uint32_t)compact_shares_needed(seq0_len);
      const uint32_t padding_start = pfb_start + pfb_count;
      if (worst_pfb_shares < pfb_count || s.nrs < padding_start || s.k * s.k < s.end_of_last ||
          (nblob == 0 && s.nrs != padding_start)) {
        s.status = kSpLayout;
        return;
      }
      SqHdr h;
      h.magic = kSqMagic;
      h.version = kSqVersion;
      h.k = s.k;
      h.n_tx = pfb_start;
      h.pad_start = padding_start;
      h.blob_start = s.nrs;
      h.blob_end = s.end_of_last;
      h.nblob = nblob;
      h.src_bytes = b.src_len;
      h.reserved = 0;
      h.seq_len[0] = seq0_len;
      h.seq_len[1] = seq1_len;
      h.nseg[0] = nseg0;
      h.nseg[1] = nseg1;
      h.nunit[0] = n_normal;
      h.nunit[1] = npfb;
      uint64_t at = sizeof(SqHdr);
      for (int q = 0; q < 2; q++) {
        h.seg_off[q] = (uint32_t)at;
        at = sp_up16(at + ((uint64_t)h.nseg[q] + 1) * 8);
        h.unit_off[q] = (uint32_t)at;
        at = sp_up16(at + (uint64_t)h.nunit[q] * 4);
      }
      h.blob_off = (uint32_t)at;
      at = sp_up16(at + (uint64_t)nblob * kSqBlobWords * 4);
      h.lit_off = (uint32_t)at;
      h.lit_bytes = lit_bytes;
      at = sp_up16(at + lit_bytes);
      h.plan_bytes = (uint32_t)at;
      s.hdr = h;
      s.plan_off = x.take(a.cursor, at);
      if (s.plan_off + at > a.arena_cap) s.status = kSpArena;
    });
    mark(5);
  }
  if (!s.status) {
    // ---- emit ----
    const SqHdr& h = s.hdr;
    uint8_t* plan = a.arena + s.plan_off;
    x.each([&](uint32_t t) {
      for (uint32_t i = t; i < h.plan_bytes / 16; i += T) {
        uint64_t* z = (uint64_t*)(plan + 16 * (uint64_t)i);
        z[0] = z[1] = 0;
      }
    });
    uint32_t* seg0 = (uint32_t*)(plan + h.seg_off[0]);
    uint32_t* seg1 = (uint32_t*)(plan + h.seg_off[1]);
    uint32_t* unit0 = (uint32_t*)(plan + h.unit_off[0]);
    uint32_t* unit1 = (uint32_t*)(plan + h.unit_off[1]);
    uint8_t* lit = plan + h.lit_off;
    x.each([&](uint32_t t) {
      if (t < kSqHeaderWords) ((uint32_t*)plan)[t] = ((const uint32_t*)&h)[t];
      if (t == 0) {
        seg0[2 * h.nseg[0]] = h.seq_len[0];
        seg1[2 * h.nseg[1]] = h.seq_len[1];
      }
      for (uint32_t i = t; i < n_normal; i += T) {
        const SpTxIn tx = a.tx[b.tx_base + i];
        const SpTxPos p = a.pos[b.tx_base + i];
        unit0[i] = p.pos;
        uint32_t sg = p.seg;
        if (i == 0 || a.tx[b.tx_base + i - 1].len) {
          seg0[2 * sg] = p.pos;
          seg0[2 * sg + 1] = kSqLitFlag | p.lit;
          sg++;
        }
        const uint32_t d = put_uvarint(lit + p.lit, tx.len);
        if (tx.len) {
          seg0[2 * sg] = p.pos + d;
          seg0[2 * sg + 1] = tx.off;
        }
      }
      for (uint32_t q = t; q < npfb; q += T) {
        const SpTxIn tx = a.tx[b.tx_base + n_normal + q];
        const SpTxCls c = a.cls[b.tx_base + n_normal + q];
        const SpTxPos p = a.pos[b.tx_base + n_normal + q];
        const SpPfb f = sp_pfb(c, blobs);
        unit1[q] = p.pos;
        // marshal_index_wrapper's bytes around the inner tx
        uint8_t* o = lit + p.lit;
        o += put_uvarint(o, f.iw);
        if (c.inner_len) {
          *o++ = 0x0a;
          o += put_uvarint(o, c.inner_len);
        }
        *o++ = 0x12;
        o += put_uvarint(o, f.packed);
        for (uint32_t j = 0; j < c.nblob; j++) o += put_uvarint(o, blobs[c.blob_at + j].start);
        *o++ = 0x1a;
        *o++ = 4;
        *o++ = 'I';
        *o++ = 'N';
        *o++ = 'D';
        *o++ = 'X';
        uint32_t sg = p.seg;
        if (q == 0) {
          seg1[2 * sg] = p.pos;
          seg1[2 * sg + 1] = kSqLitFlag | p.lit;
          sg++;
        }
        if (c.inner_len) {
          seg1[2 * sg] = p.pos + f.head;
          seg1[2 * sg + 1] = tx.off + c.inner_off;
          sg++;
          seg1[2 * sg] = p.pos + f.head + c.inner_len;
          seg1[2 * sg + 1] = kSqLitFlag | (p.lit + f.head);
        }
      }
      for (uint32_t i = t; i < nblob; i += T) {
        const SpBlobRec& r = blobs[sorted[i]];
        uint32_t* o = (uint32_t*)(plan + h.blob_off) + (uint64_t)i * kSqBlobWords;
        for (int w = 0; w < 4; w++) {
          const uint64_t le = sp_bswap64(r.key[w]);
          o[2 * w] = (uint32_t)le;
          o[2 * w + 1] = (uint32_t)(le >> 32);
        }
        o[8] = s.x[i];
        o[9] = r.shares;
        o[10] = r.data_off;
        o[11] = r.data_len;
      }
    });
    mark(6);
  }
  x.one([&] {
    SpRecord r;
    r.plan_off = s.status ? 0 : s.plan_off;
    r.src_off = b.src_off;
    r.plan_bytes = s.status ? 0 : s.hdr.plan_bytes;
    r.k = s.k;
    r.status = s.status;
    r.nblob = nblob;
    a.rec[blk] = r;
    a.status[blk] = s.status;
  });
}

// ---- the planner as host loops --------------------------------------------------
// The policy of dagpu_square_plan_emulate_host: the kSpLanes lanes of a phase
// run one after the other, a barrier is the end of the loop.
struct SpHostLanes {
  template <class F>
  void each(F&& f) {
    for (uint32_t t = 0; t < kSpLanes; t++) f(t);
  }
  template <class F>
  void one(F&& f) {
    f();
  }
  void scan(uint32_t (*v)[kSpLanes], uint32_t (*)[kSpLanes / 64]) {
    for (uint32_t j = 0; j < kSpScanVals; j++)
      for (uint32_t t = 1; t < kSpLanes; t++) v[j][t] += v[j][t - 1];
  }
  void lowest(uint32_t* p, uint32_t v) {
    if (v < *p) *p = v;
  }
  uint64_t clock() { return 0; }
  uint64_t take(unsigned long long* cursor, uint64_t bytes) {
    const uint64_t at = *cursor;
    *cursor += bytes;
    return at;
  }
};
// every block of a: classify, then the block's plan, in block order
inline void sp_emulate(const SpArgs& a, uint64_t ntx_total, SpShared& s) {
  for (uint64_t g = 0; g < ntx_total; g++) sp_classify_tx(a, g);
  SpHostLanes x;
  for (uint32_t blk = 0; blk < a.n; blk++) sp_plan_block(x, s, a, blk);
}

}  // namespace dagpu

// ---- the request tables of a batch (square_plan.hip) ------------------------------
// The checks every call over n blocks of packed txs makes of src_offs, ntx and
// tx_lens (ascending offsets inside src_bytes, the 2 GiB and 2^24 txs of a
// block, lengths that add up to each block's span), with the messages of
// dagpu_square_plan_device, and the upload they fill: SpBlockIn[n] | SpTxIn[ntx].
// src_offs and ntx are not null; n < 2^24.  ctx may be null (host executors).
#include <vector>
struct dagpu_ctx;
namespace dagpu {
int sp_tables(dagpu_ctx* ctx, size_t n, const void* src, const size_t* src_offs, size_t src_bytes, const uint32_t* ntx,
              const uint64_t* tx_lens, uint32_t max_square_size, std::vector<uint8_t>& up, uint64_t& ntx_total);
}
