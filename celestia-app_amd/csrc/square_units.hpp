// square_units.hpp -- the arithmetic of the tx index of a square: where unit
// (tx, or wrapped PFB) number i of a block lies (dagpu_square_units_device /
// _host / _emulate_host, dagpu_square_read_units_device; include/dagpu.h).  In
// the idiom of square_read.hpp: plain C++, no HIP include, the per-lane
// functions marked for both sides, so the kernels of square_units.hip, the
// host loop that emulates them and the stand-alone check program run the same
// code.
//
// The reference walks a compact sequence serially (parseRawData,
// parse_compact_shares.go:47-66; sqr_compact_units): from the first share's
// reserved bytes on, delimiter by delimiter.  Every compact share carries
// reserved bytes of its own, the byte index of the first unit that starts in
// it or 0, so each share can walk the units that start inside it -- but the
// reference never reads the reserved bytes of a continuation share, so the
// parallel walk has to prove that it agrees with the serial one.  One lane per
// share (squ_lane_walk):
//   a share whose reserved value r is not 0 is FLAGGED and is entered at byte
//   r; the lane parses delimiters as the serial walk does while the position
//   lies inside its own share, and keeps the number of units that start there,
//   its LANDING (the first position at or past its share's end where the walk
//   would go on; the position where it died when it stops inside the share) and
//   whether the landing is LIVE: the serial rules find a unit there.
// The lanes' units, taken in share order, are the serial walk's if and only if,
// for every sequence,
//   (a) the first share's reserved value is 0 or in 38 .. 511; if it is 0 the
//       serial walk finds no units, whatever later shares say, and the lanes
//       agree exactly when no later share is flagged, which (b) demands;
//   (b) every later flagged share is entered exactly where the nearest earlier
//       flagged share of the sequence landed, and that landing is live;
//   (c) every live landing falls on a share whose reserved bytes name exactly
//       that position;
//   (d) no delimiter a lane meets overflows 64 bits.
// Why: let f0 = 0 < f1 < ... be the flagged shares.  The serial walk starts
// where lane f0 is entered and visits that lane's units up to its landing L0.
// If L0 is not live the serial walk ends there, and by (b) no flagged share
// follows.  If it is live, (c) flags the share that holds L0 with entry L0; a
// flagged share between f0 and that one would have to be entered at L0 by (b),
// which does not lie in it; so that share is f1, and the argument repeats.  A
// lane may meet an overflowing delimiter the serial walk never reaches: (d)
// sends such a square to the host all the same, which is allowed (the host
// executor is the authority), never the other way round.
//
//   squ_delimiter     ParseDelimiter at one stream position, the 10-byte window
//                     running on into the next share's content
//   squ_walk          one lane's walk; hands every unit to a callback
//   squ_lane_walk     pass 1 of a lane: count, landing, live, and (a) (c) (d)
//   squ_lane_entered  pass 2: (b), from the nearest earlier flagged lane
//   squ_unit          a unit's 32-byte record
//   squ_find_seq      share -> its sequence in the scan's record table
//   squ_serial_square the host executor: sqr_compact_units per sequence
//   squ_emulate_square the device algorithm as a host loop over all shares
#pragma once
#include <vector>

#include "square_read.hpp"

namespace dagpu {

constexpr uint32_t kUnitsOk = 0, kUnitsScan = 1, kUnitsHost = 2, kUnitsOverflow = 3;
constexpr uint32_t kUnitsInvalidPair = 2;  // d_totals[2] of dagpu_square_read_units_device, beside overflow = 1

// dagpu_unit_record of include/dagpu.h (square_units.hip asserts the layout)
struct SquUnit {
  uint32_t start_share, end_share, seq, flags;
  uint64_t offset, len;
};
static_assert(sizeof(SquUnit) == 32, "unit record layout");

// What a lane leaves for the scan and for the lanes behind it: 8 bytes a share.
struct SquLane {
  uint32_t word;     // units that start in the share | kSquFlagged ..
  uint32_t landing;  // stream position, < 2^29 at the widest square
};
constexpr uint32_t kSquCount = 0xFFFFu, kSquFlagged = 1u << 16, kSquLive = 1u << 17, kSquViolation = 1u << 18,
                   kSquPfb = 1u << 19;  // the sequence's class, for the two running sums

namespace squ {

// the share of a compact sequence that holds stream position p
DAGPU_SQ_HD inline uint32_t share_of(uint32_t p) {
  return p < kSqFirstCompact ? 0 : 1 + (p - kSqFirstCompact) / kSqContCompact;
}
DAGPU_SQ_HD inline uint32_t c_off(uint32_t j) { return kSqShare - (j == 0 ? kSqFirstCompact : kSqContCompact); }
// the reserved bytes of a compact continuation share
DAGPU_SQ_HD inline uint32_t cont_reserved(const uint8_t* p) {
  return (uint32_t)p[30] << 24 | (uint32_t)p[31] << 16 | (uint32_t)p[32] << 8 | p[33];
}
DAGPU_SQ_HD inline uint32_t delim_len(uint64_t v) {
  uint32_t dl = 1;
  for (; v >= 0x80; v >>= 7) dl++;
  return dl;
}

}  // namespace squ

// ParseDelimiter (pkg/shares/utils.go:92-117) at stream position `at` of a
// compact sequence of `count` shares, share(j) -> the j-th share's 512 bytes,
// exactly as sqr_compact_units reads it from the gathered payload: 0 a unit of
// v bytes behind a delimiter of dl; 1 the walk stops (length 0, or a unit
// longer than what is left of the payload); 2 the varint overflows 64 bits.
// at < payload; reads shares share_of(at) and, when the window crosses its end,
// the one behind it, never a share >= count.
template <class Sh>
DAGPU_SQ_HD inline int squ_delimiter(const Sh& share, uint32_t count, uint32_t at, uint64_t& v, uint32_t& dl) {
  const uint32_t payload = sqr_stream_pos(true, count);
  uint32_t j = squ::share_of(at);
  const uint8_t* p = share(j) + squ::c_off(j) + (at - sqr_stream_pos(true, j));
  uint32_t end = sqr_stream_pos(true, j + 1);
  v = 0;
  bool done = false;
  for (uint32_t i = 0; i < 10 && !done; i++) {
    uint8_t b = 0;
    if (at + i < payload) {
      if (at + i == end) {
        j++;
        p = share(j) + squ::c_off(j);
        end += kSqContCompact;
      }
      b = *p++;
    }
    if (i == 9 && b > 1) return 2;
    v |= (uint64_t)(b & 0x7F) << (7 * i);
    done = b < 0x80;
  }
  if (!done) return 2;
  dl = squ::delim_len(v);
  if (v == 0 || at + dl > payload || v > payload - at - dl) return 1;
  return 0;
}

struct SquWalk {
  uint32_t count, landing;
  bool live, overflow;
};

// The walk of the lane of share j, entered at stream position `entry` (inside
// share j): unit(n, at, dl, v) for the n-th unit that starts in the share, its
// delimiter at `at`.  The last delimiter parsed is the one at the landing: it
// tells whether a unit is live there.
template <class Sh, class Unit>
DAGPU_SQ_HD inline SquWalk squ_walk(const Sh& share, uint32_t count, uint32_t j, uint32_t entry, Unit&& unit) {
  const uint32_t payload = sqr_stream_pos(true, count), end = sqr_stream_pos(true, j + 1);
  SquWalk w = {0, entry, false, false};
  uint32_t at = entry;
  while (at < payload) {
    uint64_t v;
    uint32_t dl;
    const int rc = squ_delimiter(share, count, at, v, dl);
    if (rc == 2) w.overflow = true;
    if (rc != 0) break;
    if (at >= end) {
      w.live = true;
      break;
    }
    unit(w.count, at, dl, v);
    w.count++;
    at += dl + (uint32_t)v;
  }
  w.landing = at;
  return w;
}

// Pass 1 of the lane of share j of a sequence whose first share has reserved
// value r0.  cls: kSquPfb for a PFB sequence, 0 for a tx sequence.
template <class Sh>
DAGPU_SQ_HD inline SquLane squ_lane_walk(const Sh& share, uint32_t count, uint32_t r0, uint32_t j, uint32_t cls) {
  SquLane out = {cls, 0};
  const uint32_t r = j == 0 ? r0 : squ::cont_reserved(share(j));
  if (r == 0) return out;
  out.word |= kSquFlagged;
  // the first share: (a).  A later one: no landing is there, or, behind a first
  // share that gives no data at all (Share.RawDataUsingReserved), no flagged
  // share precedes it: (b)
  if (r < squ::c_off(j) || r >= kSqShare || r0 == 0) {
    out.word |= kSquViolation;
    return out;
  }
  const SquWalk w = squ_walk(share, count, j, sqr_stream_pos(true, j) + (r - squ::c_off(j)),
                             [](uint32_t, uint32_t, uint32_t, uint64_t) {});
  out.word |= w.count;
  out.landing = w.landing;
  if (w.overflow) out.word |= kSquViolation;  // (d)
  if (w.live) {
    out.word |= kSquLive;
    const uint32_t jn = squ::share_of(w.landing);  // > j, < count: a live landing lies inside the payload
    if (squ::cont_reserved(share(jn)) != squ::c_off(jn) + (w.landing - sqr_stream_pos(true, jn)))
      out.word |= kSquViolation;  // (c)
  }
  return out;
}

// Pass 2, (b), for a flagged share j > 0 with a reserved value inside its
// content: `prev` is the lane of the nearest flagged share before it, which
// lies in the same sequence (squ_lane_walk has refused every flagged share
// behind a first share that is not flagged).
DAGPU_SQ_HD inline bool squ_lane_entered(SquLane prev, uint32_t j, uint32_t r) {
  return (prev.word & kSquLive) && prev.landing == sqr_stream_pos(true, j) + (r - squ::c_off(j));
}

// The record of the unit whose delimiter (dl bytes) starts at stream position
// `at` of sequence `seq`, whose first share is `first`.
DAGPU_SQ_HD inline SquUnit squ_unit(uint32_t first, uint32_t seq, uint32_t flags, uint32_t at, uint32_t dl, uint64_t v) {
  SquUnit u;
  u.start_share = first + squ::share_of(at);
  u.end_share = first + squ::share_of(at + dl + (uint32_t)v - 1) + 1;
  u.seq = seq;
  u.flags = flags & (kSeqTx | kSeqPfb);
  u.offset = at + dl;
  u.len = v;
  return u;
}

// The sequence that holds share s: the last of the nseq records (ascending
// first shares) that starts at or before s, or kSqrNone.  The caller checks
// that the record reaches s.
DAGPU_SQ_HD inline uint32_t squ_find_seq(const SqrRecord* rec, uint32_t nseq, uint32_t s) {
  uint32_t lo = 0, hi = nseq;  // rec[lo - 1].first <= s < rec[hi].first
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (rec[mid].first <= s)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo ? lo - 1 : kSqrNone;
}

// A compact, non-padding record whose shares lie inside the square.
DAGPU_SQ_HD inline bool squ_walkable(const SqrRecord& r, uint32_t total) {
  return !(r.flags & (kSeqSparse | kSeqPadding)) && r.count != 0 && r.first < total && r.count <= total - r.first;
}

inline void squ_summary(int32_t* out, uint32_t code, uint32_t index, uint32_t n_tx, uint32_t n_pfb, uint32_t bytes) {
  const bool table = code == kUnitsOk || code == kUnitsOverflow;
  out[0] = (int32_t)code;
  out[1] = (int32_t)index;
  out[2] = table ? (int32_t)(n_tx + n_pfb) : 0;
  out[3] = table ? (int32_t)n_tx : 0;
  out[4] = table ? (int32_t)n_pfb : 0;
  out[5] = table ? (int32_t)bytes : 0;
  out[6] = out[7] = 0;
}

// The host executor of one k x k square (rows row_pitch apart) over its scan's
// records and summary: sqr_compact_units over each non-padding compact
// sequence in order, the tx sequences' units first.  Returns 0, or what
// sqr_compact_units returns for the first sequence it refuses (*bad = that
// sequence's reserved value); the summary is zeroed then.
inline int squ_serial_square(const uint8_t* sq, uint32_t k, size_t row_pitch, const SqrRecord* rec,
                             const int32_t* scan, uint32_t seq_cap, uint32_t unit_cap, SquUnit* units,
                             int32_t* summary, uint32_t* bad) {
  const uint32_t total = k * k;
  if (scan[0] != (int32_t)kScanOk) {
    squ_summary(summary, kUnitsScan, 0, 0, 0, 0);
    return 0;
  }
  const uint32_t nseq = (uint32_t)scan[3] < seq_cap ? (uint32_t)scan[3] : seq_cap;
  std::vector<SquUnit> found[2];
  std::vector<uint8_t> stream;
  std::vector<uint64_t> off, len;
  for (uint32_t q = 0; q < nseq; q++) {
    const SqrRecord& r = rec[q];
    if (!squ_walkable(r, total)) continue;
    stream.resize(r.payload);
    for (uint32_t j = 0; j < r.count; j++) {
      const uint32_t s = r.first + j, at = sqr_stream_pos(true, j);
      memcpy(stream.data() + at, sq + (size_t)(s / k) * row_pitch + (size_t)(s % k) * kSqShare + squ::c_off(j),
             kSqShare - squ::c_off(j));
    }
    const size_t cap = r.payload / 2 + 1;  // a unit takes two bytes at least
    off.resize(cap);
    len.resize(cap);
    size_t n = 0;
    const int rc = sqr_compact_units(stream.data(), r.payload, r.reserved, off.data(), len.data(), cap, &n);
    if (rc != 0) {
      *bad = r.reserved;
      squ_summary(summary, kUnitsOk, 0, 0, 0, 0);
      return rc;
    }
    for (size_t i = 0; i < n; i++) {
      const uint32_t dl = squ::delim_len(len[i]);
      found[r.flags & kSeqPfb ? 1 : 0].push_back(squ_unit(r.first, q, r.flags, (uint32_t)off[i] - dl, dl, len[i]));
    }
  }
  uint32_t at = 0, bytes = 0;
  for (const auto& part : found)
    for (const SquUnit& u : part) {
      if (at < unit_cap) units[at] = u;
      at++;
      bytes += sqr::up16((uint32_t)u.len);
    }
  squ_summary(summary, at > unit_cap ? kUnitsOverflow : kUnitsOk, at > unit_cap ? at : 0, (uint32_t)found[0].size(),
              (uint32_t)found[1].size(), bytes);
  return 0;
}

// The shares of one sequence of a host square, as the lane functions take them.
struct SquHostShares {
  const uint8_t* sq;
  uint32_t k;
  size_t row_pitch;
  uint32_t first;
  const uint8_t* operator()(uint32_t j) const {
    const uint32_t s = first + j;
    return sq + (size_t)(s / k) * row_pitch + (size_t)(s % k) * kSqShare;
  }
};

// What the kernels of square_units.hip compute, as a host loop: pass 1 of
// every share's lane, the three running values as serial sums, pass 2 and the
// records.  Same functions, same order of the checks, same summary.
inline void squ_emulate_square(const uint8_t* sq, uint32_t k, size_t row_pitch, const SqrRecord* rec,
                               const int32_t* scan, uint32_t seq_cap, uint32_t unit_cap, SquUnit* units,
                               int32_t* summary) {
  const uint32_t total = k * k;
  if (scan[0] != (int32_t)kScanOk) {
    squ_summary(summary, kUnitsScan, 0, 0, 0, 0);
    return;
  }
  const uint32_t nseq = (uint32_t)scan[3] < seq_cap ? (uint32_t)scan[3] : seq_cap;
  std::vector<SquLane> lanes(total);
  std::vector<uint32_t> seq_of(total, kSqrNone);
  uint32_t n_class[2] = {0, 0};
  for (uint32_t s = 0; s < total; s++) {
    lanes[s] = {0, 0};
    const SqrHead h = sqr_decode_share(SquHostShares{sq, k, row_pitch, 0}(s));
    if (h.cls == kSeqSparse) continue;
    const uint32_t q = squ_find_seq(rec, nseq, s);
    if (q == kSqrNone || !squ_walkable(rec[q], total) || s - rec[q].first >= rec[q].count) continue;
    seq_of[s] = q;
    lanes[s] = squ_lane_walk(SquHostShares{sq, k, row_pitch, rec[q].first}, rec[q].count, rec[q].reserved,
                             s - rec[q].first, rec[q].flags & kSeqPfb ? kSquPfb : 0);
    n_class[lanes[s].word & kSquPfb ? 1 : 0] += lanes[s].word & kSquCount;
  }
  uint32_t before[2] = {0, 0}, violation = kSqrNone, bytes = 0;
  int64_t flagged = -1;
  for (uint32_t s = 0; s < total; s++) {
    const SquLane ln = lanes[s];
    const uint32_t q = seq_of[s], pfb = ln.word & kSquPfb ? 1 : 0;
    bool bad = ln.word & kSquViolation;
    if (q != kSqrNone) {
      const SqrRecord& r = rec[q];
      const SquHostShares share{sq, k, row_pitch, r.first};
      const uint32_t j = s - r.first;
      if ((ln.word & kSquFlagged) && !bad && j > 0)
        bad = flagged < 0 || !squ_lane_entered(lanes[(size_t)flagged], j, squ::cont_reserved(share(j)));
      if (ln.word & kSquCount) {
        const uint32_t base = pfb ? n_class[0] + before[1] : before[0];
        const uint32_t reserved = j == 0 ? r.reserved : squ::cont_reserved(share(j));
        squ_walk(share, r.count, j, sqr_stream_pos(true, j) + (reserved - squ::c_off(j)),
                 [&](uint32_t n, uint32_t at, uint32_t dl, uint64_t v) {
                   if (base + n < unit_cap) units[base + n] = squ_unit(r.first, q, r.flags, at, dl, v);
                   bytes += sqr::up16((uint32_t)v);
                 });
      }
    }
    if (bad && s < violation) violation = s;
    before[pfb] += ln.word & kSquCount;
    if (ln.word & kSquFlagged) flagged = s;
  }
  const uint32_t n = n_class[0] + n_class[1];
  if (violation != kSqrNone)
    squ_summary(summary, kUnitsHost, violation, 0, 0, 0);
  else
    squ_summary(summary, n > unit_cap ? kUnitsOverflow : kUnitsOk, n > unit_cap ? n : 0, n_class[0], n_class[1], bytes);
}

}  // namespace dagpu
