// square_write.hpp -- the square plan (dagpu_square_plan, square.cpp) and the
// function that computes one share of a planned square from the plan and the
// caller's packed txs.  The host executor (dagpu_square_plan_write_host) and
// the kernel (square_write.hip) both call sq_share_desc + sq_share_word: the
// CPU tests run the arithmetic the GPU runs.  Plain arithmetic only (no HIP
// include); every function is marked for both sides when hipcc compiles it.
//
// A plan is one relocatable blob of little-endian uint32 words, no pointers:
//
//   header  kSqHeaderWords words (SqHdr below)
//   seg[q]  for each compact sequence q (0 = txs, 1 = PFBs): nseg[q] + 1 pairs
//           (pos, src): the bytes of the sequence's delimited unit stream from
//           pos up to the next pair's pos come from src; src bit 31 set =
//           offset into the literal pool, else offset into the packed txs.
//           pos strictly increasing from 0; the last pair is (seq_len, 0).
//   unit[q] nunit[q] stream positions at which a unit (its varint delimiter)
//           starts, strictly increasing: the first one inside a share's content
//           window gives the share's reserved bytes.
//   blob    nblob records of kSqBlobWords: namespace (29 B, zero padded to 32),
//           first share, share count, data offset into the txs, data length;
//           sorted by first share.
//   lit     the literal pool: varint delimiters and IndexWrapper heads / tails.
//
// Share s of the k*k shares (pkg/square WriteSquare, pkg/shares splitters):
//   [0, n_tx)                  compact shares of sequence 0 (tx namespace)
//   [n_tx, pad_start)          compact shares of sequence 1 (PFB namespace)
//   [pad_start, blob_start)    reserved padding shares
//   [blob_start, blob_end)     blob b's sparse shares at [first_b, first_b +
//                              count_b); between them namespace padding shares
//                              in the previous blob's namespace
//   [blob_end, k*k)            tail padding shares
// A plan that dagpu_square_plan_check accepted makes every read below lie
// inside the plan, its literal pool or the first src_bytes of the txs.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define DAGPU_SQ_HD __host__ __device__
#else
#define DAGPU_SQ_HD
#endif

namespace dagpu {

constexpr uint32_t kSqMagic = 0x50515344u;  // "DSQP"
constexpr uint32_t kSqVersion = 1;
constexpr uint32_t kSqHeaderWords = 24;
constexpr uint32_t kSqBlobWords = 12;
constexpr uint32_t kSqLitFlag = 0x80000000u;
constexpr uint32_t kSqMaxWidth = 1024;  // stream positions and share indexes stay far below 2^31
constexpr uint32_t kSqShare = 512, kSqNs = 29;
constexpr uint32_t kSqFirstCompact = 474, kSqContCompact = 478;
constexpr uint32_t kSqFirstSparse = 478, kSqContSparse = 482;

struct SqHdr {
  uint32_t magic, version, k, plan_bytes;
  uint32_t n_tx, pad_start, blob_start, blob_end;  // share indexes, see above
  uint32_t seq_len[2];                             // bytes of each compact unit stream
  uint32_t nseg[2], seg_off[2];                    // seg_off etc.: byte offsets inside the plan
  uint32_t nunit[2], unit_off[2];
  uint32_t nblob, blob_off;
  uint32_t lit_off, lit_bytes;
  uint32_t src_bytes;  // bytes of packed txs the plan was made for
  uint32_t reserved;
};
static_assert(sizeof(SqHdr) == kSqHeaderWords * 4, "plan header layout");

DAGPU_SQ_HD inline uint32_t sq_compact_shares(uint32_t seq_len) {
  if (seq_len == 0) return 0;
  if (seq_len <= kSqFirstCompact) return 1;
  return 1 + (seq_len - kSqFirstCompact + kSqContCompact - 1) / kSqContCompact;
}
DAGPU_SQ_HD inline uint32_t sq_sparse_shares(uint32_t len) {
  if (len == 0) return 0;
  if (len < kSqFirstSparse) return 1;
  return 1 + (len - kSqFirstSparse + kSqContSparse - 1) / kSqContSparse;
}

// What one share is made of: hdr_len header bytes (hdr, little-endian packed,
// zero past hdr_len), then the stream bytes [c0, c_end) of its source, then
// zeros.  The source is the segment table seg[lo .. hi] (mode 1) or the txs
// bytes at direct + position (mode 2); mode 0 has no content.
struct SqShareDesc {
  uint64_t hdr[5];
  uint32_t hdr_len;
  uint32_t mode;
  uint32_t c0, c_end;
  uint32_t lo, hi;  // mode 1: first and last segment that [c0, c_end) touches
  const uint32_t* seg;
  uint32_t direct;
};

namespace sqw {

DAGPU_SQ_HD inline void put_byte(uint64_t* w, uint32_t at, uint8_t v) { w[at >> 3] |= (uint64_t)v << (8 * (at & 7)); }
DAGPU_SQ_HD inline void put_be32(uint64_t* w, uint32_t at, uint32_t v) {
  put_byte(w, at, (uint8_t)(v >> 24));
  put_byte(w, at + 1, (uint8_t)(v >> 16));
  put_byte(w, at + 2, (uint8_t)(v >> 8));
  put_byte(w, at + 3, (uint8_t)v);
}
// reserved namespaces (pkg/namespace/consts.go): `fill` 28 times, then `last`
DAGPU_SQ_HD inline void put_reserved_ns(uint64_t* w, uint8_t fill, uint8_t last) {
  const uint64_t f = 0x0101010101010101ull * fill;
  w[0] = w[1] = w[2] = f;
  w[3] = f & 0xFFFFFFFFull;
  put_byte(w, kSqNs - 1, last);
}
// index of the last pair of t[0 .. n] (pos at t[2 i]) with pos <= p; t[0] = 0 <= p
DAGPU_SQ_HD inline uint32_t seg_find(const uint32_t* t, uint32_t lo, uint32_t hi, uint32_t p) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo + 1) >> 1);
    if (t[2 * mid] <= p) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// 8 source bytes at any alignment.  The device reads the one or two aligned
// words that hold them (each holds at least one wanted byte, so each lies in a
// mapped page) and funnel-shifts; the host reads exactly the 8 bytes.
DAGPU_SQ_HD inline uint64_t load8(const uint8_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uintptr_t a = (uintptr_t)p;
  const uint64_t* q = (const uint64_t*)(a & ~(uintptr_t)7);
  const uint32_t sh = (uint32_t)(a & 7) * 8;
  const uint64_t x = q[0];
  if (sh == 0) return x;
  return (x >> sh) | (q[1] << (64 - sh));
#else
  uint64_t v;
  memcpy(&v, p, 8);
  return v;
#endif
}

}  // namespace sqw

// The make-up of share s (0 <= s < k*k) of a checked plan.
DAGPU_SQ_HD inline SqShareDesc sq_share_desc(const uint8_t* plan, uint32_t s) {
  const SqHdr& h = *(const SqHdr*)plan;
  SqShareDesc d;
  for (int i = 0; i < 5; i++) d.hdr[i] = 0;
  d.hdr_len = kSqNs + 1;
  d.mode = 0;
  d.c0 = d.c_end = d.lo = d.hi = d.direct = 0;
  d.seg = nullptr;
  if (s < h.pad_start) {  // compact share j of sequence q
    const uint32_t q = s < h.n_tx ? 0 : 1;
    const uint32_t j = q ? s - h.n_tx : s;
    sqw::put_reserved_ns(d.hdr, 0x00, q ? 0x04 : 0x01);
    d.c0 = j == 0 ? 0 : kSqFirstCompact + (j - 1) * kSqContCompact;
    const uint32_t c1 = d.c0 + (j == 0 ? kSqFirstCompact : kSqContCompact);
    d.c_end = c1 < h.seq_len[q] ? c1 : h.seq_len[q];
    d.hdr_len = kSqNs + 1 + (j == 0 ? 8 : 4);
    // reserved bytes: where the first unit that starts in this share starts
    const uint32_t* u = (const uint32_t*)(plan + h.unit_off[q]);
    uint32_t lo = 0, hi = h.nunit[q];
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (u[mid] < d.c0) lo = mid + 1; else hi = mid;
    }
    const uint32_t reserved = lo < h.nunit[q] && u[lo] < c1 ? d.hdr_len + (u[lo] - d.c0) : 0;
    // constant byte positions on both arms: the header words stay in registers
    if (j == 0) {
      sqw::put_byte(d.hdr, kSqNs, 1);  // share version 0, sequence start
      sqw::put_be32(d.hdr, kSqNs + 1, h.seq_len[q]);
      sqw::put_be32(d.hdr, kSqNs + 5, reserved);
    } else {
      sqw::put_be32(d.hdr, kSqNs + 1, reserved);
    }
    d.mode = 1;
    d.seg = (const uint32_t*)(plan + h.seg_off[q]);
    d.lo = sqw::seg_find(d.seg, 0, h.nseg[q] - 1, d.c0);
    d.hi = sqw::seg_find(d.seg, d.lo, h.nseg[q] - 1, d.c_end - 1);
    return d;
  }
  if (s < h.blob_start) {  // reserved padding
    sqw::put_reserved_ns(d.hdr, 0x00, 0xFF);
    sqw::put_byte(d.hdr, kSqNs, 1);
    return d;
  }
  if (s >= h.blob_end) {  // tail padding
    sqw::put_reserved_ns(d.hdr, 0xFF, 0xFE);
    sqw::put_byte(d.hdr, kSqNs, 1);
    return d;
  }
  // the last blob that starts at or before s
  const uint32_t* b = (const uint32_t*)(plan + h.blob_off);
  uint32_t lo = 0, hi = h.nblob - 1;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo + 1) >> 1);
    if (b[mid * kSqBlobWords + 8] <= s) lo = mid; else hi = mid - 1;
  }
  b += lo * kSqBlobWords;
  for (int i = 0; i < 4; i++) d.hdr[i] = (uint64_t)b[2 * i] | ((uint64_t)b[2 * i + 1] << 32);
  const uint32_t j = s - b[8], len = b[11];
  if (j >= b[9]) {  // namespace padding after this blob
    sqw::put_byte(d.hdr, kSqNs, 1);
    return d;
  }
  if (j == 0) {
    sqw::put_byte(d.hdr, kSqNs, 1);
    sqw::put_be32(d.hdr, kSqNs + 1, len);
    d.hdr_len = kSqNs + 5;
  }
  d.c0 = j == 0 ? 0 : kSqFirstSparse + (j - 1) * kSqContSparse;
  const uint32_t c1 = d.c0 + (j == 0 ? kSqFirstSparse : kSqContSparse);
  d.c_end = c1 < len ? c1 : len;
  d.mode = 2;
  d.direct = b[10];
  return d;
}

// Bytes [8 i, 8 i + 8) of the share (0 <= i < 64), little-endian packed.
DAGPU_SQ_HD inline uint64_t sq_share_word(const SqShareDesc& d, const uint8_t* lit, const uint8_t* src, uint32_t i) {
  const uint32_t b0 = 8 * i;
  // the header word by a chain of selects, not an indexed read: d stays in registers
  const uint64_t hw = i == 0 ? d.hdr[0] : i == 1 ? d.hdr[1] : i == 2 ? d.hdr[2] : i == 3 ? d.hdr[3] : i == 4 ? d.hdr[4] : 0;
  if (b0 + 8 <= d.hdr_len) return hw;
  uint64_t out = hw;
  const uint32_t skip = b0 < d.hdr_len ? d.hdr_len - b0 : 0;  // header bytes in this word
  const uint32_t p = d.c0 + (b0 + skip - d.hdr_len);
  if (d.mode == 0 || p >= d.c_end) return out;
  const uint32_t want = d.c_end - p < 8 - skip ? d.c_end - p : 8 - skip;
  const uint8_t* at;
  uint32_t run, sg = 0;  // run: source bytes in one piece from `at`
  if (d.mode == 2) {
    at = src + d.direct + p;
    run = d.c_end - p;
  } else {
    sg = sqw::seg_find(d.seg, d.lo, d.hi, p);
    const uint32_t from = d.seg[2 * sg + 1] + (p - d.seg[2 * sg]);
    at = from & kSqLitFlag ? lit + (from & ~kSqLitFlag) : src + from;
    run = d.seg[2 * sg + 2] - p;
  }
  if (want == 8 && run >= 8) return sqw::load8(at);
  // a seam: the header's end, a segment's end or the content's end in this word
  for (uint32_t n = 0; n < want; n++) {
    if (run == 0) {  // mode 1 only: on to the next segment
      sg++;
      const uint32_t from = d.seg[2 * sg + 1];
      at = from & kSqLitFlag ? lit + (from & ~kSqLitFlag) : src + from;
      run = d.seg[2 * sg + 2] - d.seg[2 * sg];
    }
    out |= (uint64_t)*at++ << (8 * (skip + n));
    run--;
  }
  return out;
}

}  // namespace dagpu
