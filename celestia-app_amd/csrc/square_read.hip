// square_read.hip -- squares resident in HBM read back into sequences, blobs
// and tx streams (dagpu_square_scan_device, dagpu_square_read_device;
// include/dagpu.h), the opposite direction of square_write.hip.  The arithmetic
// is square_read.hpp, shared with the host executor (dagpu_square_scan_host).
//
// Scan = shares.ParseShares(shares, false) of n squares, four launches whose
// order on the stream is the only ordering between workgroups (no workgroup
// waits for another, no look-back):
//   square_scan_local   one lane per share, 1024 shares per workgroup: 40 B of
//                       each share decoded, the start flags of a wave by
//                       __ballot, the 16 waves' counts and last starts through
//                       LDS -> per workgroup {starts, last start}
//   square_scan_carry   one wave per square over its <= 1024 workgroup
//                       summaries: starts before each workgroup and the nearest
//                       start before it; zeroes the square's accumulators
//   square_scan_emit    the local scan again with the carries: every share
//                       knows the nearest start at or before it and the number
//                       of starts before it.  Pass-1 errors and the lowest
//                       unsupported version by atomicMin; the share that ends a
//                       sequence (the next start, or the square's last share)
//                       writes its record, checks its length (pass 2, atomicMin)
//                       and adds to the square's totals (one atomicAdd per wave)
//   square_scan_final   one lane per square: the 8-word summary
// Read = select + gather:
//   square_select_partial / _carry / _emit
//                       the matching non-padding sequences of the squares whose
//                       code is OK, an exclusive scan over the whole batch of
//                       {1, payload rounded to 16, shares}: d_selected,
//                       d_offsets, d_totals, each selected sequence's first
//                       wave (share prefix) and, per wave, its sequence
//   square_gather       one wave per selected share (the grid covers every
//                       share of the batch; waves past the selected total
//                       leave at once): wave -> sequence -> record, then
//                       sqr_gather_lane per lane
// Loads: share s of square i at i * square_stride + (s / k) * row_pitch +
// (s % k) * 512, s < k * k, i < n; records and summary inside the tables the
// entry points size.  Stores: records [i * seq_cap, (i + 1) * seq_cap), the
// summary's 8 n words, and payload bytes [offset, offset + payload_len) of a
// sequence only when that end is <= payload_cap.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "runtime.hpp"
#include "square_geom.hpp"
#include "square_read.hpp"

static_assert(sizeof(dagpu_seq_record) == sizeof(dagpu::SqrRecord), "dagpu_seq_record is SqrRecord");
static_assert(offsetof(dagpu_seq_record, first_share) == offsetof(dagpu::SqrRecord, first) &&
                  offsetof(dagpu_seq_record, share_count) == offsetof(dagpu::SqrRecord, count) &&
                  offsetof(dagpu_seq_record, sequence_len) == offsetof(dagpu::SqrRecord, seq_len) &&
                  offsetof(dagpu_seq_record, flags) == offsetof(dagpu::SqrRecord, flags) &&
                  offsetof(dagpu_seq_record, reserved_bytes) == offsetof(dagpu::SqrRecord, reserved) &&
                  offsetof(dagpu_seq_record, payload_len) == offsetof(dagpu::SqrRecord, payload),
              "dagpu_seq_record is SqrRecord");
static_assert(DAGPU_SCAN_OK == dagpu::kScanOk && DAGPU_SCAN_NAMESPACE == dagpu::kScanNamespace &&
                  DAGPU_SCAN_INCONSISTENT == dagpu::kScanInconsistent && DAGPU_SCAN_LENGTH == dagpu::kScanLength &&
                  DAGPU_SCAN_OVERFLOW == dagpu::kScanOverflow && DAGPU_SEQ_SPARSE == dagpu::kSeqSparse &&
                  DAGPU_SEQ_TX == dagpu::kSeqTx && DAGPU_SEQ_PFB == dagpu::kSeqPfb &&
                  DAGPU_SEQ_PADDING == dagpu::kSeqPadding && DAGPU_SEQ_VERSION_SHIFT == dagpu::kSeqVersionShift &&
                  DAGPU_READ_BLOBS == dagpu::kReadBlobs && DAGPU_READ_COMPACT == dagpu::kReadCompact &&
                  DAGPU_SCAN_SUMMARY_WORDS == dagpu::kSqrSummaryWords,
              "include/dagpu.h and square_read.hpp agree");

namespace dagpu {

namespace {

constexpr uint32_t kScanBlock = 1024, kScanWaves = kScanBlock / 64;
// per-square accumulators of the scan, in the workspace
enum { kAccErr1, kAccErr2, kAccVer, kAccSeq, kAccBlobs, kAccBlobBytes, kAccCompactBytes, kAccWords = 8 };

// What a share knows after the scan inside its workgroup.
struct Near {
  int32_t before;  // the nearest start share strictly before this one (square index), or -1
  uint32_t rank;   // start shares strictly before this one
};

// `start`: this lane's share starts a sequence (false past the square's end);
// s: its share index.  cnt / last: 16 words of LDS each.  Returns the values
// relative to the workgroup; wg_cnt / wg_last are the workgroup's own.
__device__ inline Near scan_local(bool start, uint32_t s, uint32_t* cnt, int32_t* last, uint32_t& wg_cnt,
                                  int32_t& wg_last) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t mask = __ballot(start);
  const uint64_t below = mask & ((1ull << lane) - 1);
  Near r;
  r.rank = __popcll(below);
  r.before = below ? (int32_t)(s - lane + (63 - __clzll((long long)below))) : -1;
  if (lane == 0) {
    cnt[wave] = __popcll(mask);
    last[wave] = mask ? (int32_t)(s + (63 - __clzll((long long)mask))) : -1;
  }
  __syncthreads();
  wg_cnt = 0;
  wg_last = -1;
  for (uint32_t w = 0; w < kScanWaves; w++) {
    const uint32_t c = cnt[w];
    const int32_t l = last[w];
    if (w == wave) {
      r.rank += wg_cnt;
      if (r.before < 0) r.before = wg_last;
    }
    wg_cnt += c;
    if (l >= 0) wg_last = l;
  }
  return r;
}

}  // namespace

// grid (workgroups per square, n)
__global__ __launch_bounds__(kScanBlock) void square_scan_local(SqGeom g, uint2* __restrict__ wg_sum) {
  __shared__ uint32_t cnt[kScanWaves];
  __shared__ int32_t last[kScanWaves];
  const uint32_t sq = blockIdx.y, s = blockIdx.x * kScanBlock + threadIdx.x;
  bool start = false;
  if (s < g.total) start = load_head(share_at(g, sq, s)).start;
  uint32_t wg_cnt;
  int32_t wg_last;
  (void)scan_local(start, s, cnt, last, wg_cnt, wg_last);
  if (threadIdx.x == 0) wg_sum[(uint64_t)sq * gridDim.x + blockIdx.x] = make_uint2(wg_cnt, (uint32_t)wg_last);
}

// grid n, one wave per square
__global__ __launch_bounds__(64) void square_scan_carry(const uint2* __restrict__ wg_sum, uint2* __restrict__ wg_carry,
                                                        uint32_t wgs, uint32_t* __restrict__ acc) {
  const uint32_t sq = blockIdx.x, lane = threadIdx.x;
  uint32_t run_cnt = 0;
  int32_t run_last = -1;
  for (uint32_t base = 0; base < wgs; base += 64) {
    const uint32_t b = base + lane;
    const uint2 v = b < wgs ? wg_sum[(uint64_t)sq * wgs + b] : make_uint2(0, (uint32_t)-1);
    uint32_t c = v.x;
    int32_t l = (int32_t)v.y;
    for (uint32_t d = 1; d < 64; d <<= 1) {  // inclusive: sum of the counts, max of the last starts
      const uint32_t oc = __shfl_up(c, d);
      const int32_t ol = __shfl_up(l, d);
      if (lane >= d) {
        c += oc;
        l = ol > l ? ol : l;
      }
    }
    int32_t l_ex = __shfl_up(l, 1);
    if (lane == 0) l_ex = -1;
    if (b < wgs)
      wg_carry[(uint64_t)sq * wgs + b] = make_uint2(run_cnt + c - v.x, (uint32_t)(l_ex > run_last ? l_ex : run_last));
    const uint32_t tc = __shfl(c, 63);
    const int32_t tl = __shfl(l, 63);
    run_cnt += tc;
    run_last = tl > run_last ? tl : run_last;
  }
  if (lane < kAccWords) {
    uint32_t v = 0;
    if (lane == kAccErr1 || lane == kAccErr2 || lane == kAccVer) v = kSqrNone;
    if (lane == kAccSeq) v = run_cnt;
    acc[sq * kAccWords + lane] = v;
  }
}

namespace {

// The sequence [first, end) of square sq, the rank-th of its square: record,
// length check, totals (added to the lane's running sums).
__device__ inline void close_sequence(const SqGeom& g, uint32_t sq, uint32_t first, uint32_t end, uint32_t rank,
                                      uint32_t seq_cap, SqrRecord* __restrict__ records, uint32_t* acc,
                                      uint32_t& blobs, uint32_t& blob_bytes, uint32_t& compact_bytes) {
  SqrRecord r;
  if (!sqr_make_record(load_head(share_at(g, sq, first)), first, end - first, r))
    atomicMin(&acc[sq * kAccWords + kAccErr2], first);
  if (!(r.flags & kSeqPadding)) {
    if (r.flags & kSeqSparse) {
      blobs++;
      blob_bytes += sqr::up16(r.payload);
    } else {
      compact_bytes += sqr::up16(r.payload);
    }
  }
  if (rank < seq_cap) {
    uint4* o = (uint4*)&records[(uint64_t)sq * seq_cap + rank];
    const uint4* v = (const uint4*)&r;
    o[0] = v[0];
    o[1] = v[1];
    o[2] = v[2];
    o[3] = v[3];
  }
}

}  // namespace

// grid (workgroups per square, n)
__global__ __launch_bounds__(kScanBlock) void square_scan_emit(SqGeom g, const uint2* __restrict__ wg_carry,
                                                               uint32_t seq_cap, SqrRecord* __restrict__ records,
                                                               uint32_t* __restrict__ acc) {
  __shared__ uint32_t cnt[kScanWaves];
  __shared__ int32_t last[kScanWaves];
  const uint32_t sq = blockIdx.y, s = blockIdx.x * kScanBlock + threadIdx.x;
  const bool live = s < g.total;
  SqrHead h;
  h.start = 0;
  if (live) h = load_head(share_at(g, sq, s));
  uint32_t wg_cnt;
  int32_t wg_last;
  Near nr = scan_local(live && h.start, s, cnt, last, wg_cnt, wg_last);
  const uint2 carry = wg_carry[(uint64_t)sq * gridDim.x + blockIdx.x];
  nr.rank += carry.x;
  if (nr.before < 0) nr.before = (int32_t)carry.y;
  uint32_t blobs = 0, blob_bytes = 0, compact_bytes = 0;
  if (live) {
    uint32_t* a = acc + sq * kAccWords;
    if (h.version != 0) atomicMin(&a[kAccVer], s);
    // pass 1 (parse.go:51-75): Namespace() first, then the comparison with the
    // sequence under construction
    if (!h.ns_ok) {
      atomicMin(&a[kAccErr1], s << 2);
    } else if (!h.start) {
      bool same = nr.before >= 0;
      if (same) {
        const uint8_t* p = share_at(g, sq, (uint32_t)nr.before);
        const uint4 x = ((const uint4*)p)[0], y = ((const uint4*)p)[1];
        same = (x.x | (uint64_t)x.y << 32) == h.ns[0] && (x.z | (uint64_t)x.w << 32) == h.ns[1] &&
               (y.x | (uint64_t)y.y << 32) == h.ns[2] &&
               ((y.z | (uint64_t)y.w << 32) & 0xFFFFFFFFFFull) == h.ns[3];
      }
      if (!same) atomicMin(&a[kAccErr1], s << 2 | 1);
    }
    // a start share ends the sequence before it; the last share ends its own
    if (h.start && nr.before >= 0)
      close_sequence(g, sq, (uint32_t)nr.before, s, nr.rank - 1, seq_cap, records, acc, blobs, blob_bytes,
                     compact_bytes);
    if (s == g.total - 1) {
      const int32_t first = h.start ? (int32_t)s : nr.before;
      if (first >= 0)
        close_sequence(g, sq, (uint32_t)first, g.total, nr.rank + h.start - 1, seq_cap, records, acc, blobs,
                       blob_bytes, compact_bytes);
    }
  }
  blobs = wave_sum(blobs);
  blob_bytes = wave_sum(blob_bytes);
  compact_bytes = wave_sum(compact_bytes);
  if ((threadIdx.x & 63) == 0 && (blobs | blob_bytes | compact_bytes)) {
    uint32_t* a = acc + sq * kAccWords;
    atomicAdd(&a[kAccBlobs], blobs);
    atomicAdd(&a[kAccBlobBytes], blob_bytes);
    atomicAdd(&a[kAccCompactBytes], compact_bytes);
  }
}

__global__ __launch_bounds__(256) void square_scan_final(const uint32_t* __restrict__ acc, uint32_t n,
                                                         uint32_t seq_cap, int32_t* __restrict__ summary) {
  const uint32_t sq = blockIdx.x * 256 + threadIdx.x;
  if (sq >= n) return;
  const uint32_t* a = acc + sq * kAccWords;
  uint32_t code = kScanOk, index = 0;
  if (a[kAccErr1] != kSqrNone) {
    code = a[kAccErr1] & 1 ? kScanInconsistent : kScanNamespace;
    index = a[kAccErr1] >> 2;
  } else if (a[kAccErr2] != kSqrNone) {
    code = kScanLength;
    index = a[kAccErr2];
  } else if (a[kAccSeq] > seq_cap) {
    code = kScanOverflow;
    index = a[kAccSeq];
  }
  int4* o = (int4*)(summary + sq * kSqrSummaryWords);
  o[0] = make_int4((int)code, (int)index, a[kAccVer] == kSqrNone ? -1 : (int)a[kAccVer], (int)a[kAccSeq]);
  o[1] = make_int4((int)a[kAccBlobs], (int)a[kAccBlobBytes], (int)a[kAccCompactBytes], 0);
}

// ---- select ---------------------------------------------------------------

namespace {

struct Sel {
  uint64_t n, bytes, shares;
};

struct SelArgs {
  const SqrRecord* records;
  const int32_t* summary;
  const uint64_t* ns;  // n_ns namespaces, 4 words each
  uint64_t slots;      // n * seq_cap
  uint32_t seq_cap, n_ns, mask;
};

// slot's contribution; rec_payload / rec_count of a selected one
__device__ inline Sel select_eval(const SelArgs& a, uint64_t slot, uint32_t& payload) {
  Sel z = {0, 0, 0};
  payload = 0;
  if (slot >= a.slots) return z;
  const uint32_t sq = (uint32_t)(slot / a.seq_cap), j = (uint32_t)(slot - (uint64_t)sq * a.seq_cap);
  const int32_t* sm = a.summary + sq * kSqrSummaryWords;
  if (sm[0] != (int32_t)kScanOk || j >= (uint32_t)sm[3]) return z;
  const SqrRecord* r = a.records + slot;
  const uint32_t flags = r->flags;
  if (flags & kSeqPadding) return z;
  if (!(a.mask & (flags & kSeqSparse ? kReadBlobs : kReadCompact))) return z;
  if (a.n_ns) {
    const uint64_t n0 = r->ns[0], n1 = r->ns[1], n2 = r->ns[2], n3 = r->ns[3];
    bool hit = false;
    for (uint32_t i = 0; i < a.n_ns && !hit; i++)
      hit = a.ns[4 * i] == n0 && a.ns[4 * i + 1] == n1 && a.ns[4 * i + 2] == n2 && a.ns[4 * i + 3] == n3;
    if (!hit) return z;
  }
  payload = r->payload;
  Sel s = {1, sqr::up16(payload), r->count};
  return s;
}

// Exclusive scan of v over the 1024 lanes of the workgroup; total = the sum.
// lds: kSelLds words.  The 16 wave totals are scanned by wave 0.
constexpr uint32_t kSelLds = 3 * kScanWaves + 3;
__device__ inline Sel wave_scan(Sel v, uint32_t lane) {  // inclusive
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint64_t a = __shfl_up((unsigned long long)v.n, d), b = __shfl_up((unsigned long long)v.bytes, d),
                   c = __shfl_up((unsigned long long)v.shares, d);
    if (lane >= d) {
      v.n += a;
      v.bytes += b;
      v.shares += c;
    }
  }
  return v;
}
__device__ inline Sel block_scan(Sel v, uint64_t* lds, Sel& total) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const Sel inc = wave_scan(v, lane);
  __syncthreads();  // lds may still be read from a previous round
  if (lane == 63) {
    lds[wave] = inc.n;
    lds[kScanWaves + wave] = inc.bytes;
    lds[2 * kScanWaves + wave] = inc.shares;
  }
  __syncthreads();
  if (wave == 0) {
    Sel t = {0, 0, 0};
    if (lane < kScanWaves) t = {lds[lane], lds[kScanWaves + lane], lds[2 * kScanWaves + lane]};
    const Sel ti = wave_scan(t, lane);
    if (lane < kScanWaves) {
      lds[lane] = ti.n - t.n;
      lds[kScanWaves + lane] = ti.bytes - t.bytes;
      lds[2 * kScanWaves + lane] = ti.shares - t.shares;
    }
    if (lane == kScanWaves - 1) {
      lds[3 * kScanWaves] = ti.n;
      lds[3 * kScanWaves + 1] = ti.bytes;
      lds[3 * kScanWaves + 2] = ti.shares;
    }
  }
  __syncthreads();
  total = {lds[3 * kScanWaves], lds[3 * kScanWaves + 1], lds[3 * kScanWaves + 2]};
  return {inc.n - v.n + lds[wave], inc.bytes - v.bytes + lds[kScanWaves + wave],
          inc.shares - v.shares + lds[2 * kScanWaves + wave]};
}

}  // namespace

__global__ __launch_bounds__(kScanBlock) void square_select_partial(SelArgs a, Sel* __restrict__ partial) {
  __shared__ uint64_t lds[kSelLds];
  uint32_t payload;
  const Sel v = select_eval(a, (uint64_t)blockIdx.x * kScanBlock + threadIdx.x, payload);
  Sel total;
  (void)block_scan(v, lds, total);
  if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// one workgroup: partial[] -> its exclusive scan in place, the totals
__global__ __launch_bounds__(kScanBlock) void square_select_carry(Sel* __restrict__ partial, uint32_t blocks,
                                                                  uint64_t* __restrict__ totals,
                                                                  uint64_t* __restrict__ total_shares) {
  __shared__ uint64_t lds[kSelLds];
  Sel run = {0, 0, 0};
#pragma unroll 1
  for (uint32_t base = 0; base < blocks; base += kScanBlock) {
    const uint32_t b = base + threadIdx.x;
    Sel v = {0, 0, 0};
    if (b < blocks) v = partial[b];
    Sel total;
    const Sel ex = block_scan(v, lds, total);
    if (b < blocks) partial[b] = {run.n + ex.n, run.bytes + ex.bytes, run.shares + ex.shares};
    run = {run.n + total.n, run.bytes + total.bytes, run.shares + total.shares};
  }
  if (threadIdx.x == 0) {
    totals[0] = run.n;
    totals[1] = run.bytes;
    totals[2] = 0;
    *total_shares = run.shares;
  }
}

__global__ __launch_bounds__(kScanBlock) void square_select_emit(SelArgs a, const Sel* __restrict__ partial,
                                                                 uint64_t payload_cap, uint32_t* __restrict__ selected,
                                                                 uint64_t* __restrict__ offsets,
                                                                 uint64_t* __restrict__ share_prefix,
                                                                 uint32_t* __restrict__ share_map,
                                                                 uint64_t map_cap, uint64_t* __restrict__ totals) {
  __shared__ uint64_t lds[kSelLds];
  const uint64_t slot = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
  uint32_t payload;
  const Sel v = select_eval(a, slot, payload);
  Sel total;
  const Sel ex = block_scan(v, lds, total);
  if (!v.n) return;
  const Sel base = partial[blockIdx.x];
  const uint64_t m = base.n + ex.n, off = base.bytes + ex.bytes;
  selected[m] = (uint32_t)slot;
  offsets[m] = off;
  const uint64_t first_wave = base.shares + ex.shares;
  share_prefix[m] = first_wave;
  if (off + payload > payload_cap) totals[2] = 1;
  // the gather's wave -> sequence map.  The shares of a scan's sequences are
  // disjoint, so the waves number at most the n * k * k entries (map_cap) the
  // workspace holds; records that are no scan's stay inside it all the same.
  for (uint64_t j = 0; j < v.shares && first_wave + j < map_cap; j++) share_map[first_wave + j] = (uint32_t)m;
}

// one wave per selected share, 4 per workgroup
__global__ __launch_bounds__(256) void square_gather(SqGeom g, const SqrRecord* __restrict__ records, uint32_t seq_cap,
                                                     const uint32_t* __restrict__ selected,
                                                     const uint64_t* __restrict__ offsets,
                                                     const uint64_t* __restrict__ share_prefix,
                                                     const uint32_t* __restrict__ share_map, uint64_t map_cap,
                                                     const uint64_t* __restrict__ totals,
                                                     const uint64_t* __restrict__ total_shares,
                                                     uint8_t* __restrict__ payload, uint64_t payload_cap) {
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t w = (uint64_t)blockIdx.x * 4 + wave;
  if (w >= *total_shares || w >= map_cap) return;
  const uint32_t m = share_map[w];
  if (m >= totals[0]) return;
  const uint32_t slot = selected[m];
  const uint64_t first_wave = share_prefix[m], off = offsets[m];
  const SqrRecord* r = records + slot;
  const uint32_t len = r->payload;
  if (off + len > payload_cap) return;
  const uint32_t j = (uint32_t)(w - first_wave), s = r->first + j;
  if (j >= r->count || s >= g.total) return;
  sqr_gather_lane(share_at(g, slot / seq_cap, s), payload + off, !(r->flags & kSeqSparse), j, len, threadIdx.x & 63);
}

namespace {

uint32_t scan_wgs(uint32_t k) { return (k * k + kScanBlock - 1) / kScanBlock; }

// read workspace: namespaces | partial sums | share prefix | wave -> sequence map | total shares
struct ReadCarve {
  size_t ns, partial, prefix, map, total, bytes;
  uint32_t blocks;
};
ReadCarve read_carve(uint32_t k, size_t n, uint32_t seq_cap, size_t n_ns) {
  ReadCarve c;
  const uint64_t slots = (uint64_t)n * seq_cap;
  c.blocks = (uint32_t)((slots + kScanBlock - 1) / kScanBlock);
  c.ns = 0;
  c.partial = up16(n_ns * 32);
  c.prefix = c.partial + up16((size_t)c.blocks * sizeof(Sel));
  c.map = c.prefix + up16(slots * sizeof(uint64_t));
  c.total = c.map + up16((size_t)n * k * k * sizeof(uint32_t));
  c.bytes = c.total + 16;
  return c;
}

}  // namespace

}  // namespace dagpu

extern "C" {

size_t dagpu_square_scan_workspace_size(uint32_t k, size_t n) {
  using namespace dagpu;
  if (!is_pow2(k) || k > kSqMaxWidth) return 0;
  // workgroup summaries | carries | accumulators
  return 2 * up16(n * scan_wgs(k) * sizeof(uint2)) + up16(n * kAccWords * 4);
}

int dagpu_square_scan_host(uint32_t k, size_t n, const uint8_t* squares, size_t square_stride, size_t row_pitch,
                           uint32_t seq_cap, dagpu_seq_record* records, int32_t* summary) {
  using namespace dagpu;
  if (n == 0) return DAGPU_OK;
  if (!is_pow2(k) || k > kSqMaxWidth)
    return set_err(nullptr, DAGPU_ERR_ARG, "square width must be a power of two <= 1024");
  if (!squares || !summary || (seq_cap && !records)) return set_err(nullptr, DAGPU_ERR_ARG, "null argument");
  if (row_pitch < (size_t)k * kSS || (n > 1 && square_stride < (size_t)(k - 1) * row_pitch + (size_t)k * kSS))
    return set_err(nullptr, DAGPU_ERR_ARG, "row_pitch below k * 512 or square_stride below one square");
  for (size_t i = 0; i < n; i++)
    sqr_scan_square(squares + i * square_stride, k, row_pitch, seq_cap, (SqrRecord*)records + i * seq_cap,
                    summary + i * kSqrSummaryWords);
  return DAGPU_OK;
}

int dagpu_compact_units(const uint8_t* stream, size_t len, uint32_t first_unit, uint64_t* out_off, uint64_t* out_len,
                        size_t cap, size_t* n) {
  using namespace dagpu;
  if (!n || (len && !stream) || (cap && (!out_off || !out_len)))
    return set_err(nullptr, DAGPU_ERR_ARG, "null argument");
  const int rc = sqr_compact_units(stream, len, first_unit, out_off, out_len, cap, n);
  if (rc == 1) return set_err(nullptr, DAGPU_ERR_SQUARE, "binary: varint overflows a 64-bit integer");
  if (rc == 2)
    return set_err(nullptr, DAGPU_ERR_ARG, "reserved bytes " + std::to_string(first_unit) +
                                               " point outside the first compact share's content (38 .. 511)");
  if (*n > cap) return set_err(nullptr, DAGPU_ERR_ARG, "more units than cap");
  return DAGPU_OK;
}

int dagpu_square_scan_device(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* d_squares, size_t square_stride,
                             size_t row_pitch, uint32_t seq_cap, dagpu_seq_record* d_records, int32_t* d_summary,
                             int32_t* summary_out, void* d_workspace, void* stream) {
  using namespace dagpu;
  if (!ctx) return DAGPU_ERR_ARG;
  if (n == 0) return DAGPU_OK;
  SqGeom g;
  if (const int rc = check_geometry(ctx, k, n, d_squares, square_stride, row_pitch, d_workspace, g)) return rc;
  if (!d_summary || (seq_cap && !d_records)) return set_err(ctx, DAGPU_ERR_ARG, "null argument");
  if (((uintptr_t)d_records | (uintptr_t)d_summary) & 15)
    return set_err(ctx, DAGPU_ERR_ARG, "d_records and d_summary must be multiples of 16");
  if ((uint64_t)n * seq_cap > ((uint64_t)1 << 32))
    return set_err(ctx, DAGPU_ERR_ARG, "more than 2^32 sequence records in one call");
  hipStream_t s = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)d_workspace;
  void* own = nullptr;
  if (!ws) {
    HIP_TRY(ctx, hipMalloc(&own, dagpu_square_scan_workspace_size(k, n)));
    ws = (uint8_t*)own;
  }
  const uint32_t wgs = scan_wgs(k);
  uint2* wg_sum = (uint2*)ws;
  uint2* wg_carry = (uint2*)(ws + up16(n * wgs * sizeof(uint2)));
  uint32_t* acc = (uint32_t*)(ws + 2 * up16(n * wgs * sizeof(uint2)));
  auto run = [&]() -> int {
    const dim3 grid(wgs, (unsigned)n);
    hipLaunchKernelGGL(square_scan_local, grid, dim3(kScanBlock), 0, s, g, wg_sum);
    hipLaunchKernelGGL(square_scan_carry, dim3((unsigned)n), dim3(64), 0, s, wg_sum, wg_carry, wgs, acc);
    hipLaunchKernelGGL(square_scan_emit, grid, dim3(kScanBlock), 0, s, g, wg_carry, seq_cap, (SqrRecord*)d_records,
                       acc);
    hipLaunchKernelGGL(square_scan_final, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, acc, (uint32_t)n,
                       seq_cap, d_summary);
    HIP_TRY(ctx, hipGetLastError());
    if (summary_out) {
      HIP_TRY(ctx, hipMemcpyAsync(summary_out, d_summary, n * kSqrSummaryWords * 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(ctx, hipStreamSynchronize(s));
    }
    return DAGPU_OK;
  };
  int rc = run();
  if (own) {
    const hipError_t e = hipStreamSynchronize(s);
    if (rc == DAGPU_OK && e != hipSuccess) rc = hip_fail(ctx, e, "hipStreamSynchronize");
    (void)hipFree(own);
  }
  return rc;
}

size_t dagpu_square_read_workspace_size(uint32_t k, size_t n, uint32_t seq_cap, size_t n_ns) {
  if (!is_pow2(k) || k > dagpu::kSqMaxWidth) return 0;
  return dagpu::read_carve(k, n, seq_cap, n_ns).bytes;
}

int dagpu_square_read_device(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* d_squares, size_t square_stride,
                             size_t row_pitch, uint32_t seq_cap, const dagpu_seq_record* d_records,
                             const int32_t* d_summary, const uint8_t* namespaces, size_t n_ns, uint32_t class_mask,
                             uint32_t* d_selected, uint64_t* d_offsets, uint64_t* d_totals, uint8_t* d_payload,
                             size_t payload_cap, void* d_workspace, void* stream) {
  using namespace dagpu;
  if (!ctx) return DAGPU_ERR_ARG;
  if (n == 0) return DAGPU_OK;
  SqGeom g;
  if (const int rc = check_geometry(ctx, k, n, d_squares, square_stride, row_pitch, d_workspace, g)) return rc;
  if (!d_records || !d_summary || !d_selected || !d_offsets || !d_totals || (payload_cap && !d_payload) ||
      (n_ns && !namespaces))
    return set_err(ctx, DAGPU_ERR_ARG, "null argument");
  if (seq_cap == 0) return set_err(ctx, DAGPU_ERR_ARG, "seq_cap must be positive");
  if (class_mask == 0 || (class_mask & ~(kReadBlobs | kReadCompact)))
    return set_err(ctx, DAGPU_ERR_ARG, "class_mask must be DAGPU_READ_BLOBS, DAGPU_READ_COMPACT or both");
  if (((uintptr_t)d_records | (uintptr_t)d_summary | (uintptr_t)d_payload) & 15)
    return set_err(ctx, DAGPU_ERR_ARG, "d_records, d_summary and d_payload must be multiples of 16");
  if (((uintptr_t)d_offsets | (uintptr_t)d_totals) & 7 || (uintptr_t)d_selected & 3)
    return set_err(ctx, DAGPU_ERR_ARG, "d_offsets and d_totals must be multiples of 8, d_selected of 4");
  if ((uint64_t)n * seq_cap > ((uint64_t)1 << 32))
    return set_err(ctx, DAGPU_ERR_ARG, "more than 2^32 sequence records in one call");
  const ReadCarve c = read_carve(k, n, seq_cap, n_ns);
  std::vector<uint64_t> ns(4 * n_ns, 0);
  for (size_t i = 0; i < n_ns; i++) memcpy(&ns[4 * i], namespaces + i * kSqNs, kSqNs);
  hipStream_t s = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)d_workspace;
  void* own = nullptr;
  if (!ws) {
    HIP_TRY(ctx, hipMalloc(&own, c.bytes));
    ws = (uint8_t*)own;
  }
  hipEvent_t up = n_ns ? ev_take(ctx) : nullptr;
  auto run = [&]() -> int {
    if (n_ns) {
      if (!up) return set_err(ctx, DAGPU_ERR_DEVICE, "no event for the namespace upload");
      HIP_TRY(ctx, hipMemcpyAsync(ws + c.ns, ns.data(), n_ns * 32, hipMemcpyHostToDevice, s));
      HIP_TRY(ctx, hipEventRecord(up, s));
    }
    const SelArgs a = {(const SqrRecord*)d_records, d_summary, (const uint64_t*)(ws + c.ns), (uint64_t)n * seq_cap,
                       seq_cap, (uint32_t)n_ns, class_mask};
    Sel* partial = (Sel*)(ws + c.partial);
    uint64_t* prefix = (uint64_t*)(ws + c.prefix);
    uint32_t* share_map = (uint32_t*)(ws + c.map);
    uint64_t* total = (uint64_t*)(ws + c.total);
    hipLaunchKernelGGL(square_select_partial, dim3(c.blocks), dim3(kScanBlock), 0, s, a, partial);
    hipLaunchKernelGGL(square_select_carry, dim3(1), dim3(kScanBlock), 0, s, partial, c.blocks, d_totals, total);
    hipLaunchKernelGGL(square_select_emit, dim3(c.blocks), dim3(kScanBlock), 0, s, a, partial, (uint64_t)payload_cap,
                       d_selected, d_offsets, prefix, share_map, (uint64_t)n * g.total, d_totals);
    const uint64_t shares = (uint64_t)n * g.total;
    hipLaunchKernelGGL(square_gather, dim3((unsigned)((shares + 3) / 4)), dim3(256), 0, s, g,
                       (const SqrRecord*)d_records, seq_cap, d_selected, d_offsets, prefix, share_map, shares, d_totals, total,
                       d_payload,
                       (uint64_t)payload_cap);
    HIP_TRY(ctx, hipGetLastError());
    // the namespace table is this frame's: wait until its upload has passed
    if (n_ns) HIP_TRY(ctx, hipEventSynchronize(up));
    return DAGPU_OK;
  };
  int rc = run();
  if (own) {
    const hipError_t e = hipStreamSynchronize(s);
    if (rc == DAGPU_OK && e != hipSuccess) rc = hip_fail(ctx, e, "hipStreamSynchronize");
    (void)hipFree(own);
  } else if (rc != DAGPU_OK && n_ns) {
    (void)hipStreamSynchronize(s);
  }
  if (up) ev_give(ctx, up);
  return rc;
}

}  // extern "C"
