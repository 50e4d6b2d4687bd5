// square_read.hpp -- the arithmetic of reading a square back into sequences,
// blobs and tx streams (dagpu_square_scan_device / _host, dagpu_square_read_device,
// dagpu_compact_units; include/dagpu.h).  The mirror image of square_write.hpp
// and in its idiom: plain C++, no HIP include, every function marked for both
// sides, so the host executor, the stand-alone check program and the kernels of
// square_read.hip run the same code.
//
//   sqr_decode         the first 40 bytes of a share -> namespace, info byte,
//                      sequence length, reserved bytes, class, padding, content
//                      window (pkg/shares/shares.go:60-200)
//   sqr_shares_needed  CompactSharesNeeded / SparseSharesNeeded
//                      (share_sequence.go:106-142) over sq_compact_shares /
//                      sq_sparse_shares
//   sqr_stream_pos     where share j's content starts in its sequence's stream
//   sqr_make_record    one sequence's record and its length check
//                      (ShareSequence.validSequenceLen, share_sequence.go:54-76)
//   sqr_gather_window  one 8-B word of one share's content into the payload, of
//                      a window of the sequence's stream
//   sqr_gather_lane    the same for the whole payload
//   sqr_scan_square    the host executor: shares.ParseShares(shares, false)
//                      (parse.go:42-97) of one square, serially
//   sqr_compact_units  parseRawData (parse_compact_shares.go:47-66)
#pragma once
#include "square_write.hpp"

namespace dagpu {

constexpr uint32_t kScanOk = 0, kScanNamespace = 1, kScanInconsistent = 2, kScanLength = 3, kScanOverflow = 4;
constexpr uint32_t kSeqSparse = 1, kSeqTx = 2, kSeqPfb = 4, kSeqPadding = 8, kSeqVersionShift = 8;
constexpr uint32_t kReadBlobs = 1, kReadCompact = 2;
constexpr uint32_t kSqrHeadBytes = 40;  // what sqr_decode reads of a share
constexpr uint32_t kSqrSummaryWords = 8;
constexpr uint32_t kSqrNone = 0xFFFFFFFFu;

// dagpu_seq_record of include/dagpu.h (square_read.hip asserts the layout)
struct SqrRecord {
  uint64_t ns[4];  // the namespace's 29 bytes, zero padded to 32
  uint32_t first, count, seq_len, flags, reserved, payload;
  uint32_t pad[2];
};
static_assert(sizeof(SqrRecord) == 64, "sequence record layout");

struct SqrHead {
  uint64_t ns[4];
  uint32_t version, start;  // the info byte's two fields
  uint32_t seq_len;         // start shares; 0 on a continuation, as Share.SequenceLen
  uint32_t reserved;        // compact shares; 0 on sparse ones
  uint32_t cls;             // kSeqTx, kSeqPfb or kSeqSparse
  uint32_t ns_ok;           // namespace.From accepts the namespace
  uint32_t padding;         // Share.IsPadding
  uint32_t c_off, c_len;    // the content window
};

namespace sqr {

DAGPU_SQ_HD inline uint32_t be32(uint64_t lo, uint64_t hi, uint32_t shift) {
  // four bytes starting `shift` bits into lo (running on into hi), big-endian
  const uint32_t le = (uint32_t)(shift ? (lo >> shift) | (hi << (64 - shift)) : lo);
  return (le >> 24) | ((le >> 8) & 0xFF00u) | ((le << 8) & 0xFF0000u) | (le << 24);
}
DAGPU_SQ_HD inline uint32_t up16(uint32_t v) { return (v + 15u) & ~15u; }

}  // namespace sqr

// namespace.From (pkg/namespace/namespace.go:40-58, validateVersionSupported /
// validateID): version 0 with 18 leading zero ID bytes, or version 255.
DAGPU_SQ_HD inline bool sqr_namespace_ok(const uint64_t* ns) {
  const uint32_t v = (uint32_t)(ns[0] & 0xFF);
  if (v == 0xFF) return true;
  if (v != 0) return false;
  return (ns[0] >> 8) == 0 && ns[1] == 0 && (ns[2] & 0xFFFFFFull) == 0;
}

// w: bytes [0, 40) of the share, little-endian packed.
DAGPU_SQ_HD inline SqrHead sqr_decode(const uint64_t* w) {
  SqrHead h;
  h.ns[0] = w[0];
  h.ns[1] = w[1];
  h.ns[2] = w[2];
  h.ns[3] = w[3] & 0xFFFFFFFFFFull;
  const uint32_t info = (uint32_t)(w[3] >> 40) & 0xFF;
  h.version = info >> 1;
  h.start = info & 1;
  const bool low_zero = h.ns[0] == 0 && h.ns[1] == 0 && h.ns[2] == 0 && (h.ns[3] & 0xFFFFFFFFull) == 0;
  const uint32_t last = (uint32_t)(h.ns[3] >> 32);
  h.cls = low_zero && last == 0x01 ? kSeqTx : low_zero && last == 0x04 ? kSeqPfb : kSeqSparse;
  const bool compact = h.cls != kSeqSparse;
  h.seq_len = h.start ? sqr::be32(w[3], w[4], 48) : 0;
  h.reserved = !compact ? 0 : h.start ? sqr::be32(w[4], 0, 16) : sqr::be32(w[3], w[4], 48);
  h.ns_ok = sqr_namespace_ok(h.ns);
  const bool tail = h.ns[0] == ~0ull && h.ns[1] == ~0ull && h.ns[2] == ~0ull && h.ns[3] == 0xFEFFFFFFFFull;
  const bool res_pad = low_zero && last == 0xFF;
  h.padding = (h.start && h.seq_len == 0) || tail || res_pad;
  const uint32_t hdr = kSqNs + 1 + (h.start ? 4 : 0) + (compact ? 4 : 0);
  h.c_off = hdr;
  h.c_len = kSqShare - hdr;
  return h;
}

// The host's way to the 40 bytes (the kernels load them as 16 + 16 + 8).
inline SqrHead sqr_decode_share(const uint8_t* share) {
  uint64_t w[5];
  memcpy(w, share, kSqrHeadBytes);
  return sqr_decode(w);
}

// CompactSharesNeeded / SparseSharesNeeded.  A length no square of the widest
// supported width can hold needs more shares than any sequence has.
DAGPU_SQ_HD inline uint32_t sqr_shares_needed(uint32_t len, bool compact) {
  if (len > kSqMaxWidth * kSqMaxWidth * kSqContSparse) return kSqrNone;
  return compact ? sq_compact_shares(len) : sq_sparse_shares(len);
}

// Where the content of a sequence's share j starts in the sequence's stream.
DAGPU_SQ_HD inline uint32_t sqr_stream_pos(bool compact, uint32_t j) {
  if (j == 0) return 0;
  return compact ? kSqFirstCompact + (j - 1) * kSqContCompact : kSqFirstSparse + (j - 1) * kSqContSparse;
}

// The record of the sequence that starts with share `first` (header h) and has
// `count` shares.  Returns false where validSequenceLen refuses it.
DAGPU_SQ_HD inline bool sqr_make_record(const SqrHead& h, uint32_t first, uint32_t count, SqrRecord& r) {
  const bool compact = h.cls != kSeqSparse;
  const bool padding = count == 1 && h.padding;  // ShareSequence.isPadding
  for (int i = 0; i < 4; i++) r.ns[i] = h.ns[i];
  r.first = first;
  r.count = count;
  r.seq_len = h.seq_len;
  r.flags = h.cls | (padding ? kSeqPadding : 0) | (h.version << kSeqVersionShift);
  r.reserved = h.reserved;
  // a blob's data; a compact sequence's content windows uncut (extractRawData,
  // parse_compact_shares.go:72-86)
  r.payload = padding ? 0 : compact ? sqr_stream_pos(true, count) : h.seq_len;
  r.pad[0] = r.pad[1] = 0;
  return padding || sqr_shares_needed(h.seq_len, compact) == count;
}

// The wave that moves share j of a sequence into the payload: lane `lane`
// (0 .. 63) owns the aligned 8-B word lane of the words the share's content
// touches, counted from the sequence's base `dst` (16-B aligned).  A word that
// lies wholly inside the share's part of the stream is one (funnel-shifted)
// load and one aligned store; the two edge words, which the neighbouring
// shares' waves also write, go byte by byte.  Nothing outside the sequence's
// payload_len bytes is written.
//
// sqr_gather_window is the general form: of the sequence's stream only the
// window [w0, w0 + w_len) is wanted, and `dst` (16-B aligned) is where stream
// position w0 goes; the words are counted from there.  The whole payload is the
// window [0, payload_len); one unit of a compact sequence is the window
// [offset, offset + len) (dagpu_square_read_units_device).
DAGPU_SQ_HD inline void sqr_gather_window(const uint8_t* share, uint8_t* dst, bool compact, uint32_t j, uint32_t w0,
                                          uint32_t w_len, uint32_t lane) {
  const uint32_t c_len = j == 0 ? (compact ? kSqFirstCompact : kSqFirstSparse)
                                : (compact ? kSqContCompact : kSqContSparse);
  const uint32_t c_off = kSqShare - c_len;
  const uint32_t pos = sqr_stream_pos(compact, j);
  // the share's part of the window, in stream positions
  const uint32_t from = pos > w0 ? pos : w0, to = pos + c_len < w0 + w_len ? pos + c_len : w0 + w_len;
  if (from >= to) return;
  const uint32_t start = from - w0, end = to - w0;  // the same, counted from dst
  const uint32_t lo = ((start >> 3) + lane) << 3;
  const uint32_t a = lo > start ? lo : start, b = lo + 8 < end ? lo + 8 : end;
  if (a >= b) return;
  const uint8_t* src = share + c_off + (a + w0 - pos);
  if (b - a == 8) {
    const uint64_t v = sqw::load8(src);
#if defined(__HIP_DEVICE_COMPILE__)
    *(uint64_t*)(dst + lo) = v;
#else
    memcpy(dst + lo, &v, 8);
#endif
    return;
  }
  for (uint32_t n = 0; n < b - a; n++) dst[a + n] = src[n];
}
DAGPU_SQ_HD inline void sqr_gather_lane(const uint8_t* share, uint8_t* dst, bool compact, uint32_t j,
                                        uint32_t payload_len, uint32_t lane) {
  sqr_gather_window(share, dst, compact, j, 0, payload_len, lane);
}

// shares.ParseShares(shares, false) of one k x k square, rows row_pitch apart:
// up to seq_cap records and the 8-word summary (include/dagpu.h).
inline void sqr_scan_square(const uint8_t* sq, uint32_t k, size_t row_pitch, uint32_t seq_cap, SqrRecord* rec,
                            int32_t* summary) {
  const uint32_t total = k * k;
  auto share = [&](uint32_t i) { return sq + (size_t)(i / k) * row_pitch + (size_t)(i % k) * kSqShare; };
  uint32_t err1 = kSqrNone, err2 = kSqrNone, ver = kSqrNone;
  uint32_t nseq = 0, nblob = 0, blob_bytes = 0, compact_bytes = 0;
  int64_t cur = -1;  // the nearest start share so far
  auto close = [&](uint32_t end) {
    if (cur < 0) return;
    SqrRecord r;
    const bool ok = sqr_make_record(sqr_decode_share(share((uint32_t)cur)), (uint32_t)cur, end - (uint32_t)cur, r);
    if (!ok && err2 == kSqrNone) err2 = (uint32_t)cur;
    if (!(r.flags & kSeqPadding)) {
      if (r.flags & kSeqSparse) {
        nblob++;
        blob_bytes += sqr::up16(r.payload);
      } else {
        compact_bytes += sqr::up16(r.payload);
      }
    }
    if (nseq < seq_cap) rec[nseq] = r;
    nseq++;
  };
  for (uint32_t i = 0; i < total; i++) {
    const SqrHead h = sqr_decode_share(share(i));
    if (h.version != 0 && ver == kSqrNone) ver = i;
    uint32_t e = kSqrNone;
    if (!h.ns_ok) {
      e = i << 2;
    } else if (!h.start) {
      bool same = cur >= 0;
      if (same) {
        const SqrHead s = sqr_decode_share(share((uint32_t)cur));
        same = s.ns[0] == h.ns[0] && s.ns[1] == h.ns[1] && s.ns[2] == h.ns[2] && s.ns[3] == h.ns[3];
      }
      if (!same) e = i << 2 | 1;
    }
    if (e < err1) err1 = e;
    if (h.start) {
      close(i);
      cur = i;
    }
  }
  close(total);
  uint32_t code = kScanOk, index = 0;
  if (err1 != kSqrNone) {
    code = err1 & 1 ? kScanInconsistent : kScanNamespace;
    index = err1 >> 2;
  } else if (err2 != kSqrNone) {
    code = kScanLength;
    index = err2;
  } else if (nseq > seq_cap) {
    code = kScanOverflow;
    index = nseq;
  }
  summary[0] = (int32_t)code;
  summary[1] = (int32_t)index;
  summary[2] = ver == kSqrNone ? -1 : (int32_t)ver;
  summary[3] = (int32_t)nseq;
  summary[4] = (int32_t)nblob;
  summary[5] = (int32_t)blob_bytes;
  summary[6] = (int32_t)compact_bytes;
  summary[7] = 0;
}

// parseRawData over a compact sequence's payload (`stream`, len bytes: the
// content windows of its shares): the units from the first share's reserved
// byte index on.  Returns 0, 1 when a varint overflows 64 bits (ParseDelimiter
// fails), 2 when `reserved` points into the share's header or past it; *n is
// the number of units found, of which the first `cap` are stored.
inline int sqr_compact_units(const uint8_t* stream, size_t len, uint32_t reserved, uint64_t* out_off,
                             uint64_t* out_len, size_t cap, size_t* n) {
  *n = 0;
  if (reserved == 0) return 0;  // no unit starts in the first share (RawDataUsingReserved)
  if (reserved < kSqShare - kSqFirstCompact || reserved >= kSqShare) return 2;
  size_t at = reserved - (kSqShare - kSqFirstCompact);
  while (at < len) {
    // ParseDelimiter: a uvarint read from a window of 10 bytes, zero padded
    uint64_t v = 0;
    bool done = false;
    for (uint32_t i = 0; i < 10 && !done; i++) {
      const uint8_t b = at + i < len ? stream[at + i] : 0;
      if (i == 9 && b > 1) return 1;
      v |= (uint64_t)(b & 0x7F) << (7 * i);
      done = b < 0x80;
    }
    if (!done) return 1;
    // the reference skips the canonical length of the value, not the bytes read
    size_t dl = 1;
    for (uint64_t t = v; t >= 0x80; t >>= 7) dl++;
    if (v == 0 || at + dl > len || v > len - at - dl) return 0;
    if (*n < cap) {
      out_off[*n] = at + dl;
      out_len[*n] = v;
    }
    (*n)++;
    at += dl + (size_t)v;
  }
  return 0;
}

}  // namespace dagpu
