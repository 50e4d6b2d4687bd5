// square_units.hip -- the tx index of squares resident in HBM
// (dagpu_square_units_device, dagpu_square_read_units_device; include/dagpu.h).
// The arithmetic, and the argument why one lane per share finds the units the
// serial walk finds, is square_units.hpp, shared with the host executor
// (dagpu_square_units_host) and the host loop that emulates these kernels
// (dagpu_square_units_emulate_host).
//
// Units = four launches in the shape of the scan (square_read.hip): their order
// on the stream is the only ordering between workgroups.
//   square_units_local  one lane per share, 1024 shares per workgroup: a
//                       compact share finds its sequence in the scan's records
//                       (binary search) and walks the units that start in it
//                       (squ_lane_walk): 8 B per share {count, flags, landing};
//                       the workgroup's {tx units, PFB units, last flagged share}
//   square_units_carry  one wave per square over its workgroup summaries:
//                       the units of each class and the nearest flagged share
//                       before each workgroup; the square's accumulators
//   square_units_emit   the local scan again with the carries, from the 8 B a
//                       share left: a flagged share checks its entry against the
//                       landing of the nearest flagged share before it (b), the
//                       lowest violating share by atomicMin; a share in which
//                       units start walks again and writes their records
//   square_units_final  one lane per square: the 8-word summary
// Read units = two launches:
//   units_select        one workgroup: each pair's length from the table (0 for
//                       a pair that names no unit), the exclusive sum of the
//                       lengths rounded up to 16: d_offsets, d_totals
//   units_gather        one wave per pair over the shares the unit touches:
//                       sqr_gather_window per lane
// Loads: shares as square_read.hip addresses them, s < k * k, and only shares
// [first, first + count) of a record that squ_walkable accepts; records
// [i * seq_cap, i * seq_cap + min(n_sequences, seq_cap)); the lanes and
// summaries inside the workspace the entry points size.  Stores: unit records
// [i * unit_cap, (i + 1) * unit_cap), the summary's 8 n words, and payload bytes
// [offset, offset + len) of a unit only when that end is <= payload_cap.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "runtime.hpp"
#include "square_geom.hpp"
#include "square_units.hpp"

static_assert(sizeof(dagpu_unit_record) == sizeof(dagpu::SquUnit) &&
                  offsetof(dagpu_unit_record, start_share) == offsetof(dagpu::SquUnit, start_share) &&
                  offsetof(dagpu_unit_record, end_share) == offsetof(dagpu::SquUnit, end_share) &&
                  offsetof(dagpu_unit_record, seq) == offsetof(dagpu::SquUnit, seq) &&
                  offsetof(dagpu_unit_record, flags) == offsetof(dagpu::SquUnit, flags) &&
                  offsetof(dagpu_unit_record, offset) == offsetof(dagpu::SquUnit, offset) &&
                  offsetof(dagpu_unit_record, len) == offsetof(dagpu::SquUnit, len),
              "dagpu_unit_record is SquUnit");
static_assert(DAGPU_UNITS_OK == dagpu::kUnitsOk && DAGPU_UNITS_SCAN == dagpu::kUnitsScan &&
                  DAGPU_UNITS_HOST == dagpu::kUnitsHost && DAGPU_UNITS_OVERFLOW == dagpu::kUnitsOverflow &&
                  DAGPU_UNITS_SUMMARY_WORDS == dagpu::kSqrSummaryWords &&
                  DAGPU_READ_UNITS_INVALID == dagpu::kUnitsInvalidPair,
              "include/dagpu.h and square_units.hpp agree");

namespace dagpu {

namespace {

constexpr uint32_t kUnitsBlock = 1024, kUnitsWaves = kUnitsBlock / 64;
// per-square accumulators, in the workspace
enum { kAccViolation, kAccTx, kAccPfb, kAccBytes, kAccWords = 4 };

// The tables of a scan, as the unit kernels read them.
struct UnitsIn {
  const SqrRecord* records;
  const int32_t* summary;
  uint32_t seq_cap;
};

struct DevShares {
  const SqGeom& g;
  uint32_t sq, first;
  __device__ const uint8_t* operator()(uint32_t j) const { return share_at(g, sq, first + j); }
};

// The sequence of share s of square sq, when it is one that is walked: its
// index in the square's records, or kSqrNone.
__device__ inline uint32_t walked_seq(const SqGeom& g, const UnitsIn& in, uint32_t sq, uint32_t s) {
  const int32_t* sm = in.summary + sq * kSqrSummaryWords;
  if (sm[0] != (int32_t)kScanOk) return kSqrNone;
  const uint32_t nseq = (uint32_t)sm[3] < in.seq_cap ? (uint32_t)sm[3] : in.seq_cap;
  const SqrRecord* rec = in.records + (uint64_t)sq * in.seq_cap;
  const uint32_t q = squ_find_seq(rec, nseq, s);
  if (q == kSqrNone || !squ_walkable(rec[q], g.total) || s - rec[q].first >= rec[q].count) return kSqrNone;
  return q;
}

// What a share knows after the scan inside its workgroup.
struct Before {
  uint32_t tx, pfb;  // units of each class that start in shares strictly before this one
  int32_t flagged;   // the nearest flagged share strictly before this one (square index), or -1
};

// ln: the lane's 8 bytes (zero past the square's end); s: its share index.
// lds: 3 * kUnitsWaves words.  Returns the values relative to the workgroup;
// wg is the workgroup's own {tx, pfb, last flagged}.
__device__ inline Before units_scan_local(SquLane ln, uint32_t s, uint32_t* lds, Before& wg) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t n = ln.word & kSquCount;
  uint32_t tx = ln.word & kSquPfb ? 0 : n, pfb = ln.word & kSquPfb ? n : 0;
  const uint32_t own_tx = tx, own_pfb = pfb;
  for (uint32_t d = 1; d < 64; d <<= 1) {  // inclusive
    const uint32_t a = __shfl_up(tx, d), b = __shfl_up(pfb, d);
    if (lane >= d) {
      tx += a;
      pfb += b;
    }
  }
  const uint64_t mask = __ballot((ln.word & kSquFlagged) != 0);
  const uint64_t below = mask & ((1ull << lane) - 1);
  Before r;
  r.tx = tx - own_tx;
  r.pfb = pfb - own_pfb;
  r.flagged = below ? (int32_t)(s - lane + (63 - __clzll((long long)below))) : -1;
  if (lane == 63) {
    lds[wave] = tx;
    lds[kUnitsWaves + wave] = pfb;
    lds[2 * kUnitsWaves + wave] = mask ? s - 63 + (63 - __clzll((long long)mask)) : kSqrNone;
  }
  __syncthreads();
  wg = {0, 0, -1};
  for (uint32_t w = 0; w < kUnitsWaves; w++) {
    if (w == wave) {
      r.tx += wg.tx;
      r.pfb += wg.pfb;
      if (r.flagged < 0) r.flagged = wg.flagged;
    }
    wg.tx += lds[w];
    wg.pfb += lds[kUnitsWaves + w];
    const int32_t l = (int32_t)lds[2 * kUnitsWaves + w];
    if (l >= 0) wg.flagged = l;
  }
  return r;
}

}  // namespace

// grid (workgroups per square, n)
__global__ __launch_bounds__(kUnitsBlock) void square_units_local(SqGeom g, UnitsIn in, SquLane* __restrict__ lanes,
                                                                  uint4* __restrict__ wg_sum) {
  __shared__ uint32_t lds[3 * kUnitsWaves];
  const uint32_t sq = blockIdx.y, s = blockIdx.x * kUnitsBlock + threadIdx.x;
  SquLane ln = {0, 0};
  if (s < g.total) {
    if (load_head(share_at(g, sq, s)).cls != kSeqSparse) {
      const uint32_t q = walked_seq(g, in, sq, s);
      if (q != kSqrNone) {
        const SqrRecord* r = in.records + (uint64_t)sq * in.seq_cap + q;
        const uint32_t first = r->first;
        ln = squ_lane_walk(DevShares{g, sq, first}, r->count, r->reserved, s - first, r->flags & kSeqPfb ? kSquPfb : 0);
      }
    }
    *(uint2*)&lanes[(uint64_t)sq * g.total + s] = make_uint2(ln.word, ln.landing);
  }
  Before wg;
  (void)units_scan_local(ln, s, lds, wg);
  if (threadIdx.x == 0)
    wg_sum[(uint64_t)sq * gridDim.x + blockIdx.x] = make_uint4(wg.tx, wg.pfb, (uint32_t)wg.flagged, 0);
}

// grid n, one wave per square
__global__ __launch_bounds__(64) void square_units_carry(const uint4* __restrict__ wg_sum,
                                                         uint4* __restrict__ wg_carry, uint32_t wgs,
                                                         uint32_t* __restrict__ acc) {
  const uint32_t sq = blockIdx.x, lane = threadIdx.x;
  uint32_t run_tx = 0, run_pfb = 0;
  int32_t run_last = -1;
  for (uint32_t base = 0; base < wgs; base += 64) {
    const uint32_t b = base + lane;
    const uint4 v = b < wgs ? wg_sum[(uint64_t)sq * wgs + b] : make_uint4(0, 0, (uint32_t)-1, 0);
    uint32_t tx = v.x, pfb = v.y;
    int32_t l = (int32_t)v.z;
    for (uint32_t d = 1; d < 64; d <<= 1) {  // inclusive: sums of the counts, max of the last flagged shares
      const uint32_t a = __shfl_up(tx, d), c = __shfl_up(pfb, d);
      const int32_t ol = __shfl_up(l, d);
      if (lane >= d) {
        tx += a;
        pfb += c;
        l = ol > l ? ol : l;
      }
    }
    int32_t l_ex = __shfl_up(l, 1);
    if (lane == 0) l_ex = -1;
    if (b < wgs)
      wg_carry[(uint64_t)sq * wgs + b] =
          make_uint4(run_tx + tx - v.x, run_pfb + pfb - v.y, (uint32_t)(l_ex > run_last ? l_ex : run_last), 0);
    const int32_t tl = __shfl(l, 63);
    run_tx += __shfl(tx, 63);
    run_pfb += __shfl(pfb, 63);
    run_last = tl > run_last ? tl : run_last;
  }
  if (lane == 0) *(uint4*)&acc[sq * kAccWords] = make_uint4(kSqrNone, run_tx, run_pfb, 0);
}

// grid (workgroups per square, n)
__global__ __launch_bounds__(kUnitsBlock) void square_units_emit(SqGeom g, UnitsIn in,
                                                                 const SquLane* __restrict__ lanes,
                                                                 const uint4* __restrict__ wg_carry, uint32_t unit_cap,
                                                                 SquUnit* __restrict__ units,
                                                                 uint32_t* __restrict__ acc) {
  __shared__ uint32_t lds[3 * kUnitsWaves];
  const uint32_t sq = blockIdx.y, s = blockIdx.x * kUnitsBlock + threadIdx.x;
  SquLane ln = {0, 0};
  if (s < g.total) {
    const uint2 v = *(const uint2*)&lanes[(uint64_t)sq * g.total + s];
    ln = {v.x, v.y};
  }
  Before wg;
  Before at = units_scan_local(ln, s, lds, wg);
  const uint4 carry = wg_carry[(uint64_t)sq * gridDim.x + blockIdx.x];
  at.tx += carry.x;
  at.pfb += carry.y;
  if (at.flagged < 0) at.flagged = (int32_t)carry.z;
  uint32_t bytes = 0;
  // only a walked share is flagged or has units: its sequence is found as in pass 1
  const uint32_t q = ln.word & (kSquFlagged | kSquCount) ? walked_seq(g, in, sq, s) : kSqrNone;
  if (q != kSqrNone) {
    const SqrRecord* r = in.records + (uint64_t)sq * in.seq_cap + q;
    const uint32_t first = r->first, count = r->count, flags = r->flags, j = s - first;
    const DevShares share{g, sq, first};
    const uint32_t reserved = j == 0 ? r->reserved : squ::cont_reserved(share(j));
    bool bad = ln.word & kSquViolation;
    if (!bad && j > 0) {  // (b)
      bad = at.flagged < 0;
      if (!bad) {
        const uint2 p = *(const uint2*)&lanes[(uint64_t)sq * g.total + (uint32_t)at.flagged];
        bad = !squ_lane_entered({p.x, p.y}, j, reserved);
      }
    }
    if (bad) atomicMin(&acc[sq * kAccWords + kAccViolation], s);
    if (ln.word & kSquCount) {
      const uint32_t base = ln.word & kSquPfb ? acc[sq * kAccWords + kAccTx] + at.pfb : at.tx;
      SquUnit* out = units + (uint64_t)sq * unit_cap;
      squ_walk(share, count, j, sqr_stream_pos(true, j) + (reserved - squ::c_off(j)),
               [&](uint32_t n, uint32_t pos, uint32_t dl, uint64_t v) {
                 if (base + n < unit_cap) {
                   const SquUnit u = squ_unit(first, q, flags, pos, dl, v);
                   uint4* o = (uint4*)&out[base + n];
                   o[0] = make_uint4(u.start_share, u.end_share, u.seq, u.flags);
                   o[1] = make_uint4((uint32_t)u.offset, (uint32_t)(u.offset >> 32), (uint32_t)u.len,
                                     (uint32_t)(u.len >> 32));
                 }
                 bytes += sqr::up16((uint32_t)v);
               });
    }
  }
  bytes = wave_sum(bytes);
  if ((threadIdx.x & 63) == 0 && bytes) atomicAdd(&acc[sq * kAccWords + kAccBytes], bytes);
}

__global__ __launch_bounds__(256) void square_units_final(const uint32_t* __restrict__ acc,
                                                          const int32_t* __restrict__ scan, uint32_t n,
                                                          uint32_t unit_cap, int32_t* __restrict__ summary) {
  const uint32_t sq = blockIdx.x * 256 + threadIdx.x;
  if (sq >= n) return;
  const uint4 a = *(const uint4*)&acc[sq * kAccWords];
  const uint32_t units = a.y + a.z;
  uint32_t code = kUnitsOk, index = 0;
  if (scan[sq * kSqrSummaryWords] != (int32_t)kScanOk) {
    code = kUnitsScan;
  } else if (a.x != kSqrNone) {
    code = kUnitsHost;
    index = a.x;
  } else if (units > unit_cap) {
    code = kUnitsOverflow;
    index = units;
  }
  const bool table = code == kUnitsOk || code == kUnitsOverflow;
  int4* o = (int4*)(summary + sq * kSqrSummaryWords);
  o[0] = make_int4((int)code, (int)index, table ? (int)units : 0, table ? (int)a.y : 0);
  o[1] = make_int4(table ? (int)a.z : 0, table ? (int)a.w : 0, 0, 0);
}

// ---- read units -----------------------------------------------------------

namespace {

struct PairArgs {
  const uint32_t* pairs;  // m {square, unit}
  const SquUnit* units;
  const int32_t* unit_summary;
  uint64_t m;
  uint32_t n, unit_cap;
};

// the unit a pair names, or nullptr
__device__ inline const SquUnit* pair_unit(const PairArgs& a, uint64_t t, uint32_t& sq) {
  sq = a.pairs[2 * t];
  const uint32_t u = a.pairs[2 * t + 1];
  if (sq >= a.n) return nullptr;
  const int32_t* sm = a.unit_summary + sq * kSqrSummaryWords;
  if (sm[0] != (int32_t)kUnitsOk || u >= (uint32_t)sm[2] || u >= a.unit_cap) return nullptr;
  return a.units + (uint64_t)sq * a.unit_cap + u;
}

}  // namespace

// one workgroup
__global__ __launch_bounds__(kUnitsBlock) void units_select(PairArgs a, uint64_t payload_cap,
                                                            uint64_t* __restrict__ offsets,
                                                            uint64_t* __restrict__ totals) {
  __shared__ uint64_t sums[kUnitsWaves];
  __shared__ uint32_t flags;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) flags = 0;
  uint64_t run = 0;
  uint32_t mine = 0;
#pragma unroll 1
  for (uint64_t base = 0; base < a.m; base += kUnitsBlock) {
    const uint64_t t = base + threadIdx.x;
    uint64_t len = 0;
    if (t < a.m) {
      uint32_t sq;
      const SquUnit* u = pair_unit(a, t, sq);
      if (u)
        len = u->len;
      else
        mine |= kUnitsInvalidPair;
    }
    uint64_t inc = (len + 15) & ~(uint64_t)15;
    const uint64_t own = inc;
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const uint64_t o = __shfl_up((unsigned long long)inc, d);
      if (lane >= d) inc += o;
    }
    __syncthreads();  // sums may still be read from the round before
    if (lane == 63) sums[wave] = inc;
    __syncthreads();
    uint64_t off = run + inc - own;
    for (uint32_t w = 0; w < kUnitsWaves; w++) {
      if (w < wave) off += sums[w];
      run += sums[w];
    }
    if (t < a.m) {
      offsets[t] = off;
      if (off + len > payload_cap) mine |= 1;
    }
  }
  if (mine) atomicOr(&flags, mine);
  __syncthreads();
  if (threadIdx.x == 0) {
    totals[0] = a.m;
    totals[1] = run;
    totals[2] = flags;
  }
}

// one wave per pair, 4 per workgroup
__global__ __launch_bounds__(256) void units_gather(SqGeom g, const SqrRecord* __restrict__ records, uint32_t seq_cap,
                                                    PairArgs a, const uint64_t* __restrict__ offsets,
                                                    uint8_t* __restrict__ payload, uint64_t payload_cap) {
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t t = (uint64_t)blockIdx.x * 4 + wave;
  if (t >= a.m) return;
  uint32_t sq;
  const SquUnit* u = pair_unit(a, t, sq);
  if (!u) return;
  const uint64_t off = offsets[t], len = u->len, from = u->offset;
  const uint32_t seq = u->seq;
  if (len == 0 || off + len > payload_cap || seq >= seq_cap) return;
  const SqrRecord* r = records + (uint64_t)sq * seq_cap + seq;
  if (!squ_walkable(*r, g.total) || from + len > r->payload) return;
  const uint32_t first = r->first;
  const uint32_t j1 = squ::share_of((uint32_t)(from + len - 1));
  for (uint32_t j = squ::share_of((uint32_t)from); j <= j1; j++)
    sqr_gather_window(share_at(g, sq, first + j), payload + off, true, j, (uint32_t)from, (uint32_t)len,
                      threadIdx.x & 63);
}

namespace {

uint32_t units_wgs(uint32_t k) { return (k * k + kUnitsBlock - 1) / kUnitsBlock; }

// units workspace: lanes | workgroup summaries | carries | accumulators
struct UnitsCarve {
  size_t lanes, sum, carry, acc, bytes;
};
UnitsCarve units_carve(uint32_t k, size_t n) {
  UnitsCarve c;
  c.lanes = 0;
  c.sum = up16(n * k * k * sizeof(SquLane));
  c.carry = c.sum + up16(n * units_wgs(k) * sizeof(uint4));
  c.acc = c.carry + up16(n * units_wgs(k) * sizeof(uint4));
  c.bytes = c.acc + up16(n * kAccWords * 4);
  return c;
}

int units_host_args(uint32_t k, size_t n, const uint8_t* squares, size_t square_stride, size_t row_pitch,
                    uint32_t seq_cap, const dagpu_seq_record* records, const int32_t* summary, uint32_t unit_cap,
                    const dagpu_unit_record* units, const int32_t* unit_summary) {
  if (!is_pow2(k) || k > kSqMaxWidth)
    return set_err(nullptr, DAGPU_ERR_ARG, "square width must be a power of two <= 1024");
  if (!squares || !summary || !unit_summary || (seq_cap && !records) || (unit_cap && !units))
    return set_err(nullptr, DAGPU_ERR_ARG, "null argument");
  if (row_pitch < (size_t)k * kSS || (n > 1 && square_stride < (size_t)(k - 1) * row_pitch + (size_t)k * kSS))
    return set_err(nullptr, DAGPU_ERR_ARG, "row_pitch below k * 512 or square_stride below one square");
  return DAGPU_OK;
}

}  // namespace

}  // namespace dagpu

extern "C" {

size_t dagpu_square_units_workspace_size(uint32_t k, size_t n) {
  using namespace dagpu;
  if (!is_pow2(k) || k > kSqMaxWidth) return 0;
  return units_carve(k, n).bytes;
}

int dagpu_square_units_host(uint32_t k, size_t n, const uint8_t* squares, size_t square_stride, size_t row_pitch,
                            uint32_t seq_cap, const dagpu_seq_record* records, const int32_t* summary,
                            uint32_t unit_cap, dagpu_unit_record* units, int32_t* unit_summary) {
  using namespace dagpu;
  if (n == 0) return DAGPU_OK;
  if (const int rc = units_host_args(k, n, squares, square_stride, row_pitch, seq_cap, records, summary, unit_cap,
                                     units, unit_summary))
    return rc;
  for (size_t i = 0; i < n; i++) {
    uint32_t bad = 0;
    const int rc = squ_serial_square(squares + i * square_stride, k, row_pitch, (const SqrRecord*)records + i * seq_cap,
                                     summary + i * kSqrSummaryWords, seq_cap, unit_cap,
                                     (SquUnit*)units + i * unit_cap, unit_summary + i * kSqrSummaryWords, &bad);
    if (rc == 1) return set_err(nullptr, DAGPU_ERR_SQUARE, "binary: varint overflows a 64-bit integer");
    if (rc == 2)
      return set_err(nullptr, DAGPU_ERR_ARG, "reserved bytes " + std::to_string(bad) +
                                                 " point outside the first compact share's content (38 .. 511)");
  }
  return DAGPU_OK;
}

int dagpu_square_units_emulate_host(uint32_t k, size_t n, const uint8_t* squares, size_t square_stride,
                                    size_t row_pitch, uint32_t seq_cap, const dagpu_seq_record* records,
                                    const int32_t* summary, uint32_t unit_cap, dagpu_unit_record* units,
                                    int32_t* unit_summary) {
  using namespace dagpu;
  if (n == 0) return DAGPU_OK;
  if (const int rc = units_host_args(k, n, squares, square_stride, row_pitch, seq_cap, records, summary, unit_cap,
                                     units, unit_summary))
    return rc;
  for (size_t i = 0; i < n; i++)
    squ_emulate_square(squares + i * square_stride, k, row_pitch, (const SqrRecord*)records + i * seq_cap,
                       summary + i * kSqrSummaryWords, seq_cap, unit_cap, (SquUnit*)units + i * unit_cap,
                       unit_summary + i * kSqrSummaryWords);
  return DAGPU_OK;
}

int dagpu_square_units_device(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* d_squares, size_t square_stride,
                              size_t row_pitch, uint32_t seq_cap, const dagpu_seq_record* d_records,
                              const int32_t* d_summary, uint32_t unit_cap, dagpu_unit_record* d_units,
                              int32_t* d_unit_summary, int32_t* unit_summary_out, void* d_workspace, void* stream) {
  using namespace dagpu;
  if (!ctx) return DAGPU_ERR_ARG;
  if (n == 0) return DAGPU_OK;
  SqGeom g;
  if (const int rc = check_geometry(ctx, k, n, d_squares, square_stride, row_pitch, d_workspace, g)) return rc;
  if (!d_summary || !d_unit_summary || (seq_cap && !d_records) || (unit_cap && !d_units))
    return set_err(ctx, DAGPU_ERR_ARG, "null argument");
  if (((uintptr_t)d_records | (uintptr_t)d_summary | (uintptr_t)d_units | (uintptr_t)d_unit_summary) & 15)
    return set_err(ctx, DAGPU_ERR_ARG, "d_records, d_summary, d_units and d_unit_summary must be multiples of 16");
  if ((uint64_t)n * seq_cap > ((uint64_t)1 << 32))
    return set_err(ctx, DAGPU_ERR_ARG, "more than 2^32 sequence records in one call");
  hipStream_t s = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)d_workspace;
  void* own = nullptr;
  const UnitsCarve c = units_carve(k, n);
  if (!ws) {
    HIP_TRY(ctx, hipMalloc(&own, c.bytes));
    ws = (uint8_t*)own;
  }
  const uint32_t wgs = units_wgs(k);
  SquLane* lanes = (SquLane*)(ws + c.lanes);
  uint4* wg_sum = (uint4*)(ws + c.sum);
  uint4* wg_carry = (uint4*)(ws + c.carry);
  uint32_t* acc = (uint32_t*)(ws + c.acc);
  const UnitsIn in = {(const SqrRecord*)d_records, d_summary, seq_cap};
  auto run = [&]() -> int {
    const dim3 grid(wgs, (unsigned)n);
    hipLaunchKernelGGL(square_units_local, grid, dim3(kUnitsBlock), 0, s, g, in, lanes, wg_sum);
    hipLaunchKernelGGL(square_units_carry, dim3((unsigned)n), dim3(64), 0, s, wg_sum, wg_carry, wgs, acc);
    hipLaunchKernelGGL(square_units_emit, grid, dim3(kUnitsBlock), 0, s, g, in, lanes, wg_carry, unit_cap,
                       (SquUnit*)d_units, acc);
    hipLaunchKernelGGL(square_units_final, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, acc, d_summary,
                       (uint32_t)n, unit_cap, d_unit_summary);
    HIP_TRY(ctx, hipGetLastError());
    if (unit_summary_out) {
      HIP_TRY(ctx, hipMemcpyAsync(unit_summary_out, d_unit_summary, n * kSqrSummaryWords * 4, hipMemcpyDeviceToHost, s));
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

size_t dagpu_square_read_units_workspace_size(size_t m) { return dagpu::up16(m * 8) + 16; }

int dagpu_square_read_units_device(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* d_squares,
                                   size_t square_stride, size_t row_pitch, uint32_t seq_cap,
                                   const dagpu_seq_record* d_records, uint32_t unit_cap,
                                   const dagpu_unit_record* d_units, const int32_t* d_unit_summary,
                                   const uint32_t* pairs, size_t m, uint64_t* d_offsets, uint64_t* d_totals,
                                   uint8_t* d_payload, size_t payload_cap, void* d_workspace, void* stream) {
  using namespace dagpu;
  if (!ctx) return DAGPU_ERR_ARG;
  if (n == 0) return DAGPU_OK;
  SqGeom g;
  if (const int rc = check_geometry(ctx, k, n, d_squares, square_stride, row_pitch, d_workspace, g)) return rc;
  if (!d_records || !d_units || !d_unit_summary || !d_totals || (m && (!pairs || !d_offsets)) ||
      (payload_cap && !d_payload))
    return set_err(ctx, DAGPU_ERR_ARG, "null argument");
  if (seq_cap == 0 || unit_cap == 0) return set_err(ctx, DAGPU_ERR_ARG, "seq_cap and unit_cap must be positive");
  if (((uintptr_t)d_records | (uintptr_t)d_units | (uintptr_t)d_unit_summary | (uintptr_t)d_payload) & 15)
    return set_err(ctx, DAGPU_ERR_ARG, "d_records, d_units, d_unit_summary and d_payload must be multiples of 16");
  if (((uintptr_t)d_offsets | (uintptr_t)d_totals) & 7)
    return set_err(ctx, DAGPU_ERR_ARG, "d_offsets and d_totals must be multiples of 8");
  if ((uint64_t)m > ((uint64_t)1 << 32) - 4) return set_err(ctx, DAGPU_ERR_ARG, "more than 2^32 units in one call");
  hipStream_t s = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)d_workspace;
  void* own = nullptr;
  if (!ws) {
    HIP_TRY(ctx, hipMalloc(&own, dagpu_square_read_units_workspace_size(m)));
    ws = (uint8_t*)own;
  }
  hipEvent_t up = m ? ev_take(ctx) : nullptr;
  auto run = [&]() -> int {
    if (m) {
      if (!up) return set_err(ctx, DAGPU_ERR_DEVICE, "no event for the upload of the pairs");
      HIP_TRY(ctx, hipMemcpyAsync(ws, pairs, m * 8, hipMemcpyHostToDevice, s));
      HIP_TRY(ctx, hipEventRecord(up, s));
    }
    const PairArgs a = {(const uint32_t*)ws, (const SquUnit*)d_units, d_unit_summary, (uint64_t)m, (uint32_t)n, unit_cap};
    hipLaunchKernelGGL(units_select, dim3(1), dim3(kUnitsBlock), 0, s, a, (uint64_t)payload_cap, d_offsets, d_totals);
    if (m)
      hipLaunchKernelGGL(units_gather, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, s, g, (const SqrRecord*)d_records,
                         seq_cap, a, d_offsets, d_payload, (uint64_t)payload_cap);
    HIP_TRY(ctx, hipGetLastError());
    // the pairs are this frame's caller's: wait until their upload has passed
    if (m) HIP_TRY(ctx, hipEventSynchronize(up));
    return DAGPU_OK;
  };
  int rc = run();
  if (own) {
    const hipError_t e = hipStreamSynchronize(s);
    if (rc == DAGPU_OK && e != hipSuccess) rc = hip_fail(ctx, e, "hipStreamSynchronize");
    (void)hipFree(own);
  } else if (rc != DAGPU_OK && m) {
    (void)hipStreamSynchronize(s);
  }
  if (up) ev_give(ctx, up);
  return rc;
}

}  // extern "C"
