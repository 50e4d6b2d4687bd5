// repair_host.cpp -- host side of Repair (include/dagpu.h dagpu_repair*): the
// workspace, the crossword's rounds and their host decisions, the exact-order
// replay that names a byzantine axis, and started (asynchronous) repairs.  The
// kernels are in repair.hip and the RS codecs; the workspace layout is
// repair_layout.hpp, the replay's plan crossword_plan.hpp.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/dagpu.h"
#include "crossword_plan.hpp"
#include "kernels.hpp"
#include "repair_layout.hpp"
#include "runtime.hpp"

using namespace dagpu;

namespace {

struct RepairWs {
  SquareArgs sa;        // NMT verification (roots of the repaired square)
  uint8_t* p0;          // presence before repair
  int32_t* complete_before;
  int32_t* complete_now;
  int32_t* root_bad;    // [axis][sq][idx]: complete-before axis whose root differs
  int32_t* parity_bad;  // [axis][sq][idx]: complete-before axis whose parity != Encode(data)
  uint8_t* err_rows;
  uint8_t* err_cols;
  int32_t* flags_rows;
  int32_t* flags_cols;
  int32_t* err_share[2][2];  // [axis][same, head]
  int32_t* sel;         // exact-order repair: level of each axis' attempt, [2][w]
  int32_t* bits;
  int32_t* counters;    // kCtrSlots round counters (kernels.hpp kCtr*)
  // fill route / deferral (repair.hip PlanArgs)
  int32_t* fill;        // [sq][idx] of the round's axis
  int32_t* pair_list;   // k = 128 fill pairs, n * w entries
  int32_t* pair_list_rev;  // k = 128 reverse fill pairs, n * w entries
  int32_t* known;       // [axis][sq][idx]
  int32_t* deferred;    // [axis][sq][idx]
  int32_t* nodefer;     // [sq]
  int32_t* check;       // [sq]: a deferred axis is not a codeword
  int32_t* counts[2];   // [axis] vec_counts: present data shards | present shards << 16
};

static_assert(kCtrSlots * sizeof(int32_t) == kRepairCounterBytes, "repair_layout.hpp: the counters region");

// The workspace regions as pointers: repair_layout.hpp's offsets plus the base.
RepairWs carve_repair(uint32_t k, size_t n, void* base) {
  const RepairLayout L = repair_layout((int)k, n);
  uint8_t* const b = (uint8_t*)base;
  auto i32 = [&](const WsRegion& g) { return (int32_t*)(b + g.off); };
  RepairWs r{};
  r.sa.k = (int)k;
  r.sa.nsq = (long)n;
  nmt_workspace_carve(r.sa, b);  // L.nmt, at offset 0
  r.sa.row_roots = b + L.row_roots.off;
  r.sa.col_roots = b + L.col_roots.off;
  r.sa.dah = b + L.dah.off;
  r.sa.status = i32(L.status);
  r.p0 = b + L.p0.off;
  r.complete_before = i32(L.complete_before);
  r.complete_now = i32(L.complete_now);
  r.root_bad = i32(L.root_bad);
  r.parity_bad = i32(L.parity_bad);
  r.err_rows = b + L.err_rows.off;
  r.err_cols = b + L.err_cols.off;
  r.flags_rows = i32(L.flags_rows);
  r.flags_cols = i32(L.flags_cols);
  for (int ax = 0; ax < 2; ax++)
    for (int j = 0; j < 2; j++) r.err_share[ax][j] = i32(L.err_share[ax][j]);
  r.sel = i32(L.sel);
  r.bits = i32(L.bits);
  r.counters = i32(L.counters);
  r.fill = i32(L.fill);
  r.pair_list = i32(L.pair_list);
  r.pair_list_rev = i32(L.pair_list_rev);
  r.known = i32(L.known);
  r.deferred = i32(L.deferred);
  r.nodefer = i32(L.nodefer);
  r.check = i32(L.check);
  r.counts[0] = i32(L.counts[0]);
  r.counts[1] = i32(L.counts[1]);
  return r;
}

DecodeArgs axis_decode_args(uint32_t k, size_t n, uint8_t* eds, uint8_t* present, int axis,
                            const RepairWs& r) {
  const long w = 2L * k;
  DecodeArgs d{};
  d.data = eds;
  d.sq_stride = (long)eds_bytes(k);
  d.present = present;
  d.p_sq_stride = w * w;
  if (axis == 0) {
    d.vec_stride = w * (long)kSS; d.shard_stride = kSS;
    d.p_vec_stride = w; d.p_shard_stride = 1;
    d.err = r.err_rows; d.flags = r.flags_rows; d.ndecodable = r.counters + kCtrRowsDec;
    d.nfill = r.counters + kCtrFillRows;
  } else {
    d.vec_stride = kSS; d.shard_stride = w * (long)kSS;
    d.p_vec_stride = 1; d.p_shard_stride = w;
    d.err = r.err_cols; d.flags = r.flags_cols; d.ndecodable = r.counters + kCtrColsDec;
    d.nfill = r.counters + kCtrFillCols;
  }
  d.err_key = r.err_share[axis][0];
  d.err_head = r.err_share[axis][1];
#ifdef DAGPU_TEST_HOOKS
  static const bool collide = getenv("DAGPU_TEST_KEY_COLLIDE") != nullptr;  // read once
  d.key_collide = collide ? 1 : 0;
#endif
  d.nsq = (long)n;
  d.nvec = w;
  d.nchunk = 1;
  d.shard_bytes = kSS;
  d.k = (int)k;
  return d;
}

}  // namespace

// The encoder's view of the same geometry: the data half of every vector of
// the axis in, its parity half out, in place in n resident EDS.
EncodeArgs dagpu::axis_encode_args(uint32_t k, size_t n, uint8_t* d_eds, int axis) {
  const long w = 2L * k;
  EncodeArgs e{};
  e.in = d_eds;
  e.in_sq_stride = e.out_sq_stride = (long)eds_bytes(k);
  if (axis == 0) {
    e.in_vec_stride = e.out_vec_stride = w * (long)kSS;
    e.in_shard_stride = e.out_shard_stride = kSS;
    e.out = d_eds + (long)k * kSS;
  } else {
    e.in_vec_stride = e.out_vec_stride = kSS;
    e.in_shard_stride = e.out_shard_stride = w * (long)kSS;
    e.out = d_eds + (long)k * w * kSS;
  }
  e.nsq = (long)n;
  e.nvec = w;
  e.nchunk = 1;
  e.shard_bytes = kSS;
  return e;
}

namespace {

std::string go_bytes(const uint8_t* p, size_t n) {  // fmt %v of a []byte
  std::string s = "[";
  for (size_t i = 0; i < n; i++) {
    if (i) s += ' ';
    s += std::to_string(p[i]);
  }
  return s + "]";
}

// Square `sq` of a batch whose parallel crossword found a rebuilt axis with the
// wrong root: rerun it in rsmt2d's sequential order to name the axis rsmt2d
// reports.  Every rebuild that verifies restores committed bytes, so up to the
// first failing attempt the batched level order fills exactly the cells
// rsmt2d's order fills, with the same bytes; an attempt's result is final once
// its axis (and the orthogonal axes it completes) are full, so one root pass at
// the end decides every attempt.  Leaves present[] as rsmt2d leaves it (cells
// of the attempts before the failing one) and byz[4] = {axis, index, rebuilt
// axis, rebuilt index}.  Synchronises `s`.
int exact_repair(dagpu_ctx* ctx, uint32_t k, size_t sq, uint8_t* d_eds, uint8_t* d_present,
                 const uint8_t* d_rr, const uint8_t* d_cr, int32_t* d_byz, const RepairWs& r,
                 hipStream_t s) {
  const size_t w = 2 * (size_t)k;
  uint8_t* eds = d_eds + sq * eds_bytes(k);
  uint8_t* pres = d_present + sq * w * w;
  std::vector<uint8_t> p0(w * w);
  HIP_TRY(ctx, hipMemcpyAsync(p0.data(), r.p0 + sq * w * w, w * w, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  const CrossPlan pl = plan_crossword((int)k, p0.data());
  HIP_TRY(ctx, hipMemcpyAsync(pres, r.p0 + sq * w * w, w * w, hipMemcpyDeviceToDevice, s));
  HIP_TRY(ctx, hipMemcpyAsync(r.sel, pl.att_level.data(), 2 * w * 4, hipMemcpyHostToDevice, s));
  std::vector<uint8_t> has(2 * (size_t)pl.nlevels, 0);
  for (size_t j = 0; j < pl.axis.size(); j++) has[2 * (size_t)pl.level[j] + pl.axis[j]] = 1;
  for (int L = 0; L < pl.nlevels; L++) {
    for (int ax = 0; ax < 2; ax++) {
      if (!has[2 * (size_t)L + ax]) continue;
      DecodeArgs d = axis_decode_args(k, 1, eds, pres, ax, r);
      d.err_key = d.err_head = nullptr;
      d.ndecodable = nullptr;
      d.sel_level = r.sel + (size_t)ax * w;
      d.sel_value = L;
      HIP_TRY(ctx, launch_rs_errlocs(d, s));
      HIP_TRY(ctx, launch_rs_decode_only(d, s, true));
    }
  }
  int rc = enqueue_roots(ctx, k, 1, eds, r.sa.row_roots, r.sa.col_roots, nullptr, r.sa.status, r.sa.digests, s);
  if (rc) return rc;
  std::vector<uint8_t> got(2 * w * kNodeSize), want(2 * w * kNodeSize);
  HIP_TRY(ctx, hipMemcpyAsync(got.data(), r.sa.row_roots, w * kNodeSize, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipMemcpyAsync(got.data() + w * kNodeSize, r.sa.col_roots, w * kNodeSize, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipMemcpyAsync(want.data(), d_rr + sq * w * kNodeSize, w * kNodeSize, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipMemcpyAsync(want.data() + w * kNodeSize, d_cr + sq * w * kNodeSize, w * kNodeSize,
                              hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  auto bad = [&](int ax, int i) {
    const size_t off = ((size_t)ax * w + i) * kNodeSize;
    return memcmp(got.data() + off, want.data() + off, kNodeSize) != 0;
  };
  int32_t byz[4] = {-1, -1, -1, -1};
  size_t fail = pl.axis.size();
  for (size_t j = 0; j < pl.axis.size() && fail == pl.axis.size(); j++) {
    const int ax = pl.axis[j], i = pl.idx[j];
    if (bad(ax, i)) {
      byz[0] = byz[2] = ax;
      byz[1] = byz[3] = i;
      fail = j;
      break;
    }
    for (int o = pl.ortho_off[j]; o < pl.ortho_off[j + 1]; o++)
      if (bad(1 - ax, pl.ortho[o])) {
        byz[0] = 1 - ax;
        byz[1] = pl.ortho[o];
        byz[2] = ax;
        byz[3] = i;
        fail = j;
        break;
      }
  }
  if (fail < pl.axis.size()) {  // presence as rsmt2d leaves it: attempts before the failing one
    std::vector<uint8_t> p = p0;
    for (size_t j = 0; j < fail; j++)
      for (size_t t = 0; t < w; t++) {
        const size_t cell = pl.axis[j] == 0 ? (size_t)pl.idx[j] * w + t : t * w + pl.idx[j];
        p[cell] = 1;
      }
    HIP_TRY(ctx, hipMemcpyAsync(pres, p.data(), w * w, hipMemcpyHostToDevice, s));
  }
  HIP_TRY(ctx, hipMemcpyAsync(d_byz + 4 * sq, byz, sizeof byz, hipMemcpyHostToDevice, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  return DAGPU_OK;
}

// A page-locked mailbox for the round counters (RAII; back to the context's pool).
struct Mailbox {
  dagpu_ctx* c;
  void* p = nullptr;
  Mailbox(const Mailbox&) = delete;
  Mailbox(Mailbox&& o) noexcept : c(o.c), p(o.p) { o.p = nullptr; }
  explicit Mailbox(dagpu_ctx* c_) : c(c_) {
    if (!c) return;  // (an empty mailbox: read_small then copies straight to the destination)
    {
      std::lock_guard<std::mutex> g(c->mb_mu);
      if (!c->mailboxes.empty()) {
        p = c->mailboxes.back();
        c->mailboxes.pop_back();
        return;
      }
    }
    if (hipHostMalloc(&p, dagpu_ctx::kMailbox, hipHostMallocDefault) != hipSuccess) p = nullptr;
  }
  ~Mailbox() {
    if (!p) return;
    std::lock_guard<std::mutex> g(c->mb_mu);
    c->mailboxes.push_back(p);
  }
};

// Small device->host read that the next host decision waits for: into the
// mailbox when there is one (a direct DMA), then a spin on the stream (the
// blocking wait's wake-up cost 50-200 us per Repair round, profiles/
// repair_timeline_r03.txt).
hipError_t read_small(void* dst, const void* src, size_t bytes, Mailbox& mb, hipStream_t s) {
  void* via = (mb.p && bytes <= dagpu_ctx::kMailbox) ? mb.p : dst;
  hipError_t e = hipMemcpyAsync(via, src, bytes, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = wait_stream(s, true);
  if (e == hipSuccess && via != dst) memcpy(dst, via, bytes);
  return e;
}

// The round counters a vec_count_round launch left in the mailbox: spin on its
// sequence word (kernels queued behind that launch keep the stream busy, so
// the stream itself is not waited for); the stream is polled now and then, for
// errors and for a word that never arrives (then the counters are copied).
hipError_t wait_round_counters(int32_t* cnt, const RoundCounters& rc, Mailbox& mb, hipStream_t s) {
  const volatile int32_t* word = rc.host + kCtrRead;
  for (unsigned spin = 0;; spin++) {
    if (*word == rc.seq) {
      __atomic_thread_fence(__ATOMIC_ACQUIRE);
      memcpy(cnt, (const void*)rc.host, kCtrRead * sizeof(int32_t));
      return hipSuccess;
    }
    if ((spin & 1023) == 1023) {
      const hipError_t e = hipStreamQuery(s);
      if (e == hipSuccess && *word != rc.seq) return read_small(cnt, rc.ctr, kCtrRead * sizeof(int32_t), mb, s);
      if (e != hipSuccess && e != hipErrorNotReady) return e;
    }
    __builtin_ia32_pause();
  }
}

std::atomic<int32_t> g_round_seq{1};

// What the steps of one repair_device call share.
struct RepairRun {
  dagpu_ctx* ctx;
  uint32_t k;
  size_t n;
  long w;  // 2k
  uint8_t* d_eds;
  uint8_t* d_present;
  hipStream_t s;
  RepairWs r;
  Mailbox* mb;
  RoundCounters rcnt;
  int64_t* stats_out;  // a started Repair's slot; NULL: the context's, under prof_mu
  bool shortcut;       // fill route and deferral (DAGPU_REPAIR_FILL=0 turns them off)
  bool fill_list;      // k = 128: the fills may run bit-sliced over pair lists
  DecodeArgs d[2];     // the round's row and column args, built anew every round
  int64_t rounds_run = 0, deferred_run = 0;  // over both passes (dagpu_repair_stats)
  long deferred_total = 0;                   // of the current pass
  int last_ax = -1;                          // axis of the pass's previous round
};

// prerepairSanityCheck: complete axes must satisfy parity == Encode(data).
// Queued after the first round's counter read, and only when some axis is
// complete (a complete axis is never written by the crossword, so the order
// does not matter; the maximal erasure patterns have none).
int prerepair_compare(RepairRun& q) {
  for (int axis = 0; axis < 2; axis++) {
    EncodeArgs e = axis_encode_args(q.k, q.n, q.d_eds, axis);
    e.vec_flags = q.r.complete_before + (long)axis * q.n * q.w;
    e.mismatch = q.r.bits;
    e.mismatch_bit = 0;
    e.mismatch_vec = q.r.parity_bad + (long)axis * q.n * q.w;
    HIP_TRY(q.ctx, launch_rs_encode((int)q.k, e, q.s));
  }
  return DAGPU_OK;
}

// Schedule totals so far (diagnostics): plans of the earlier rounds are
// complete; a started Repair writes its slot's copy (published at its join).
void publish_stats(RepairRun& q, const int32_t* cnt) {
  std::unique_lock<std::mutex> g(q.ctx->prof_mu, std::defer_lock);
  if (!q.stats_out) g.lock();
  int64_t* st = q.stats_out ? q.stats_out : q.ctx->rep_stats;
  st[0] = q.rounds_run;
  st[1] = cnt[kCtrPlan];
  st[2] = cnt[kCtrPlan + 1];
  st[3] = cnt[kCtrPlan + 2];
  st[4] = q.deferred_run + cnt[kCtrDeferred];
}

// Fill-mode encode of the round's axis: a parity shard is stored only where
// it is not present, and a given one that differs sends its vector to the
// decoder (redo = the axis' decode flags).
EncodeArgs fill_encode_args(const RepairRun& q, int ax) {
  EncodeArgs e = axis_encode_args(q.k, q.n, q.d_eds, ax);
  e.op_sq_stride = q.w * q.w;
  if (ax == 0) {
    e.out_present = q.d_present + q.k; e.op_vec_stride = q.w; e.op_shard_stride = 1;
  } else {
    e.out_present = q.d_present + (long)q.k * q.w; e.op_vec_stride = 1; e.op_shard_stride = q.w;
  }
  e.redo = q.d[ax].flags;
  return e;
}

// The round's plan (repair.hip PlanArgs): which decodable vectors of the axis
// are filled forward, filled in reverse, decoded or deferred.
int round_plan(RepairRun& q, int ax, bool listed) {
  const RepairWs& r = q.r;
  PlanArgs pa{};
  pa.counts = q.d[ax].vec_counts;
  pa.flags = q.d[ax].flags;
  pa.fill = r.fill;
  pa.pair_list = listed ? r.pair_list : nullptr;
  pa.pair_count = r.counters + kCtrPairs;
  pa.pair_list_rev = listed ? r.pair_list_rev : nullptr;
  pa.pair_count_rev = r.counters + kCtrPairsRev;
  pa.known = r.known;
  pa.deferred = r.deferred;
  pa.nodefer = r.nodefer;
  pa.ndeferred = r.counters + kCtrDeferred;
  pa.nplan = r.counters + kCtrPlan;
  pa.k = (int)q.k;
  pa.nsq = (long)q.n;
  pa.axis = ax;
  HIP_TRY(q.ctx, launch_repair_plan(pa, q.s));
  return DAGPU_OK;
}

// The round's forward fills, then its reverse fills (e: fill_encode_args).
int round_fills(RepairRun& q, EncodeArgs e, bool listed) {
  const RepairWs& r = q.r;
  ProfScope p(q.ctx, 6, q.s);
  // reverse fills: parity half in, data half out (its presence k shards before)
  EncodeArgs er = e;
  er.in = e.out;
  er.out = (uint8_t*)e.in;
  er.out_present = e.out_present - (long)q.k * e.op_shard_stride;
  er.reverse = 1;
  if (listed) {
    e.pair_list = r.pair_list;
    e.pair_count = r.counters + kCtrPairs;
    HIP_TRY(q.ctx, launch_leo8_fill_sliced(e, (long)q.n * q.w / 2, q.s));
    er.pair_list = r.pair_list_rev;
    er.pair_count = r.counters + kCtrPairsRev;
    HIP_TRY(q.ctx, launch_leo8_fill_sliced(er, (long)q.n * q.w / 2, q.s));
  } else {
    e.vec_flags = er.vec_flags = r.fill;
    e.vec_flag_match = 1;
    er.vec_flag_match = 2;
    HIP_TRY(q.ctx, launch_rs_encode((int)q.k, e, q.s));
    HIP_TRY(q.ctx, launch_rs_encode((int)q.k, er, q.s));
  }
  return DAGPU_OK;
}

// solveCrossword: each round rebuilds every decodable row or every decodable
// column (whichever set is larger) until no axis can make progress
// (*more = false: this round found none, and queued nothing after its count).
// Per round: one launch counts both axes and leaves the counters in the
// mailbox (RoundCounters), the host picks the axis, and the round's last
// launch (launch_rs_mark_round) clears the next round's counts: no memsets
// or copies between the kernels of a round.
// Fill route and deferral (repair.hip PlanArgs; DAGPU_REPAIR_FILL=0 turns
// them off): a decodable vector whose data half is complete is re-encoded
// instead of decoded, and one whose parity half is complete is rebuilt by the
// reverse transform (EncodeArgs.reverse); both give the decoder's bytes
// whenever the vector's given shards agree with them, and a vector whose
// given shards disagree goes to the decoder; when every vector i < k of an
// axis is decodable or complete, the decodes of i >= k wait and the next round
// (the other axis) fills everything.  For the maximal erasure pattern (Q3
// given) that is k reverse row fills, k reverse column fills and k row fills
// instead of k + 2k decodes.  A deferred vector the decoder would have rebuilt
// is the same codeword whenever the square ends up a codeword square, which
// the known[] bookkeeping proves for that pattern; otherwise a compare-mode
// encode checks every deferred vector, and a square that fails is re-run from
// its original presence without deferral (the decoders read present shards
// only): deferral_check.
int crossword_round(RepairRun& q, bool first, bool* more) {
  dagpu_ctx* const ctx = q.ctx;
  const RepairWs& r = q.r;
  hipStream_t s = q.s;
  *more = false;
  // decodable vectors and counts of both axes (no locators yet)
  for (int axis = 0; axis < 2; axis++) {
    q.d[axis] = axis_decode_args(q.k, q.n, q.d_eds, q.d_present, axis, r);
    q.d[axis].vec_counts = r.counts[axis];
  }
  q.rcnt.seq = g_round_seq.fetch_add(1) & 0x7fffffff;
  HIP_TRY(ctx, launch_vec_count_round(q.d[0], q.d[1], q.rcnt, s));
  // Few vectors (a launch is mostly latency): both axes' candidate locator
  // heads while the host reads the counts; else the chosen axis' after it.
  const bool early_heads = (long)q.n * q.w <= 8192;
  if (early_heads) HIP_TRY(ctx, launch_errloc_heads2(q.d[0], &q.d[1], s));
  int32_t cnt[kCtrRead] = {};
  if (q.rcnt.host) {
    HIP_TRY(ctx, wait_round_counters(cnt, q.rcnt, *q.mb, s));
  } else {
    HIP_TRY(ctx, read_small(cnt, r.counters, sizeof cnt, *q.mb, s));
  }
  cnt[kCtrDeferred] = cnt[kCtrDeferredPrev];  // the previous round's plan
  publish_stats(q, cnt);
  if (first && cnt[kCtrComplete] > 0) {
    const int prc = prerepair_compare(q);
    if (prc) return prc;
  }
  q.deferred_total += cnt[kCtrDeferred];
  q.deferred_run += cnt[kCtrDeferred];
  if (cnt[kCtrRowsDec] == 0 && cnt[kCtrColsDec] == 0) return DAGPU_OK;
  q.rounds_run++;
  int ax = cnt[kCtrRowsDec] >= cnt[kCtrColsDec] ? 0 : 1;
  // after a deferral the other axis is the one with complete data halves
  if (cnt[kCtrDeferred] > 0 && q.last_ax >= 0 && cnt[kCtrRowsDec + 1 - q.last_ax] > 0) ax = 1 - q.last_ax;
  q.last_ax = ax;
  DecodeArgs& d = q.d[ax];
  if (q.shortcut) {
    const EncodeArgs e = fill_encode_args(q, ax);
    const bool listed = q.fill_list && leo8_fill_sliced_applicable(e);
    int rc = round_plan(q, ax, listed);
    if (rc) return rc;
    // no fill candidates on this axis (the count launch's tally of the
    // plan's f / r vectors): the two fill launches would find nothing
    if (cnt[ax == 0 ? kCtrFillRows : kCtrFillCols] > 0 && (rc = round_fills(q, e, listed))) return rc;
  }
  // locators of the vectors left to the decoder (fill redos included)
  d.locators_only = 1;
  if (!early_heads) HIP_TRY(ctx, launch_errloc_heads2(d, nullptr, s));
  HIP_TRY(ctx, launch_rs_errlocs_only(d, s));
  {
    ProfScope p(ctx, 5, s);
    HIP_TRY(ctx, launch_rs_decode_only(d, s, false));
  }
  HIP_TRY(ctx, launch_rs_mark_round(d, q.shortcut ? r.fill : nullptr,
                                    q.shortcut ? r.known + (long)ax * q.n * q.w : nullptr, r.counters, s));
  *more = true;
  return DAGPU_OK;
}

// After a pass that deferred vectors: those whose codeword property is not
// implied get compare-mode encodes, and a square that fails one goes back to
// its original presence with deferral off (*rerun: run the crossword again).
int deferral_check(RepairRun& q, bool* rerun) {
  dagpu_ctx* const ctx = q.ctx;
  const RepairWs& r = q.r;
  hipStream_t s = q.s;
  const size_t n = q.n, ww = (size_t)q.w * q.w;
  *rerun = false;
  HIP_TRY(ctx, launch_repair_defer_check(r.deferred, r.known, (int)q.k, (long)n, r.check, s,
                                         r.counters + kCtrDeferSquares));
  int32_t left = 0;  // squares whose deferred axes are not proven codewords
  HIP_TRY(ctx, read_small(&left, r.counters + kCtrDeferSquares, sizeof left, *q.mb, s));
  if (left == 0) return DAGPU_OK;
  for (int axis = 0; axis < 2; axis++) {
    EncodeArgs e = axis_encode_args(q.k, n, q.d_eds, axis);
    e.vec_flags = r.deferred + (long)axis * n * q.w;
    e.mismatch = r.check;
    e.mismatch_bit = 1;
    HIP_TRY(ctx, launch_rs_encode((int)q.k, e, s));
  }
  std::vector<int32_t> chk(n);
  HIP_TRY(ctx, read_small(chk.data(), r.check, n * sizeof(int32_t), *q.mb, s));
  for (size_t i = 0; i < n; i++) {
    if (!chk[i]) continue;
    *rerun = true;
    HIP_TRY(ctx, hipMemcpyAsync(q.d_present + i * ww, r.p0 + i * ww, ww, hipMemcpyDeviceToDevice, s));
    HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)(r.nodefer + i), 1, 1, s));
  }
  return DAGPU_OK;
}

// Verify every complete axis against the given roots; status and byz[] per square.
int verify_and_finalize(RepairRun& q, const uint8_t* d_rr, const uint8_t* d_cr, int32_t* d_status,
                        int32_t* d_byz) {
  dagpu_ctx* const ctx = q.ctx;
  RepairWs& r = q.r;
  hipStream_t s = q.s;
  HIP_TRY(ctx, launch_axis_complete(q.d_present, (int)q.k, (long)q.n, r.complete_now, s));
  r.sa.eds = q.d_eds;
  r.sa.eds_sq_stride = (long)eds_bytes(q.k);
  int rc = enqueue_roots(ctx, q.k, q.n, q.d_eds, r.sa.row_roots, r.sa.col_roots, nullptr, r.sa.status,
                         r.sa.digests, s);
  if (rc) return rc;
  HIP_TRY(ctx, launch_verify_roots(d_rr, d_cr, r.sa.row_roots, r.sa.col_roots, r.complete_now,
                                   r.complete_before, (int)q.k, (long)q.n, r.bits, r.root_bad, s));
  HIP_TRY(ctx, launch_finalize_repair(r.bits, r.complete_before, r.root_bad, r.parity_bad, (int)q.k, (long)q.n,
                                      d_status, d_byz, s, r.check));
  // a square failing prerepairSanityCheck is left as its input (rsmt2d never
  // reaches solveCrossword for it): presence back to p0; the bytes of cells
  // not present are unspecified, as they are for any missing cell
  HIP_TRY(ctx, launch_restore_presence(q.d_present, r.p0, r.check, (int)q.k, (long)q.n, s));
  return DAGPU_OK;
}

// rsmt2d Repair for n same-k squares resident on the device (see repair.hip).
// d_byz (optional, n * 4 int32): failing axis per square; asking for it makes
// the call resolve crossword failures in rsmt2d's order (exact_repair).
// mb_in (optional): a mailbox the caller took already (the asynchronous path
// allocates nothing on its worker thread: an allocation there could wait for
// a stream that is itself waiting for the worker).
int repair_device(dagpu_ctx* ctx, uint32_t k, size_t n, uint8_t* d_eds, uint8_t* d_present,
                  const uint8_t* d_rr, const uint8_t* d_cr, int32_t* d_status, int32_t* d_byz, void* d_ws,
                  hipStream_t s, Mailbox* mb_in = nullptr, int64_t* stats_out = nullptr) {
  const long w = 2L * k;
  const RepairWs r = carve_repair(k, n, d_ws);
  HIP_TRY(ctx, hipMemcpyAsync(r.p0, d_present, n * w * w, hipMemcpyDeviceToDevice, s));
  HIP_TRY(ctx, hipMemsetAsync(r.bits, 0, n * sizeof(int32_t), s));
  HIP_TRY(ctx, hipMemsetAsync(r.parity_bad, 0, n * 2 * w * sizeof(int32_t), s));
  HIP_TRY(ctx, hipMemsetAsync(r.counters, 0, kCtrSlots * sizeof(int32_t), s));  // kernels.hpp kCtr*
  HIP_TRY(ctx, launch_axis_complete(d_present, (int)k, (long)n, r.complete_before, s, r.counters + kCtrComplete));
  const char* fill_env = sw(SW_REPAIR_FILL);  // read per call (tests compare both)
  const bool shortcut = !(fill_env && fill_env[0] == '0');
  if (shortcut) {
    HIP_TRY(ctx, hipMemcpyAsync(r.known, r.complete_before, n * 2 * w * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    HIP_TRY(ctx, hipMemsetAsync(r.deferred, 0, n * 2 * w * sizeof(int32_t), s));
    HIP_TRY(ctx, hipMemsetAsync(r.nodefer, 0, n * sizeof(int32_t), s));
  }
  const int max_rounds = 4 * (int)w + 4;
  Mailbox mb_own(mb_in ? nullptr : ctx);
  Mailbox& mb = mb_in ? *mb_in : mb_own;
  RepairRun q{ctx, k, n, w, d_eds, d_present, s, r, &mb,
              RoundCounters{r.counters, mb.p ? (int32_t*)mb.p : nullptr, 0}, stats_out, shortcut, k == 128};
  for (int pass = 0; pass < 2; pass++) {
    q.deferred_total = 0;
    q.last_ax = -1;
    if (pass > 0) {  // (the repair's first memset covers pass 0)
      HIP_TRY(ctx, hipMemsetAsync(r.counters, 0, (kCtrPairsRev + 1) * sizeof(int32_t), s));
      HIP_TRY(ctx, hipMemsetAsync(r.counters + kCtrDeferSquares, 0, 2 * sizeof(int32_t), s));  // and DeferredPrev
    }
    bool more = true;
    for (int round = 0; round < max_rounds && more; round++) {
      const int rc = crossword_round(q, pass == 0 && round == 0, &more);
      if (rc) return rc;
    }
    if (!shortcut || q.deferred_total == 0) break;
    bool rerun = false;
    const int rc = deferral_check(q, &rerun);
    if (rc) return rc;
    if (!rerun) break;
  }
  int rc = verify_and_finalize(q, d_rr, d_cr, d_status, d_byz);
  if (rc) return rc;
  if (!d_byz) return DAGPU_OK;
  // crossword failures: name the axis in rsmt2d's order (rare; synchronises)
  std::vector<int32_t> st(n), bz(4 * n);
  HIP_TRY(ctx, hipMemcpyAsync(st.data(), d_status, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipMemcpyAsync(bz.data(), d_byz, 4 * n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  for (size_t i = 0; i < n; i++) {
    if (st[i] != DAGPU_ERR_BYZANTINE || bz[4 * i] >= 0) continue;
    rc = exact_repair(ctx, k, i, d_eds, d_present, d_rr, d_cr, d_byz, q.r, s);
    if (rc) return rc;
  }
  return DAGPU_OK;
}

hipError_t async_init_slot(dagpu_ctx::AsyncSlot& sl) {
  hipError_t e = hipSuccess;
  if (!sl.stream && (e = hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking)) != hipSuccess) return e;
  if (!sl.fork && (e = hipEventCreateWithFlags(&sl.fork, hipEventDisableTiming)) != hipSuccess) return e;
  if (!sl.finished && (e = hipEventCreateWithFlags(&sl.finished, hipEventDisableTiming)) != hipSuccess) return e;
  return e;
}

}  // namespace

extern "C" {

size_t dagpu_repair_workspace_size(uint32_t k, size_t n) {
  if (k == 0 || n == 0) return 256;
  return repair_ws_bytes(k, n) + 256;
}

int dagpu_repair_batch_device_ex(dagpu_ctx* ctx, uint32_t k, size_t n, uint8_t* d_eds,
                                 uint8_t* d_present, const uint8_t* d_row_roots,
                                 const uint8_t* d_col_roots, int32_t* d_status, int32_t* d_byz,
                                 void* d_workspace, void* stream) {
  if (!ctx || !d_eds || !d_present || !d_row_roots || !d_col_roots || !d_status || !d_workspace)
    return DAGPU_ERR_ARG;
  int rc = check_k(ctx, k);
  if (rc) return rc;
  if (n == 0) return DAGPU_OK;
  return repair_device(ctx, k, n, d_eds, d_present, d_row_roots, d_col_roots, d_status, d_byz, d_workspace,
                       (hipStream_t)stream);
}


// Asynchronous Repair: the crossword's host decisions (one counter read per
// round) run on a library worker thread that queues the kernels on a stream
// of its own, forked from `stream` at the call; dagpu_repair_join then makes a
// stream wait for the finished repair.  Nothing on the device ever waits for
// work queued later: a first design whose caller stream waited on a signal
// word the worker would write later (hipStreamWaitValue32) hung inside the
// test suite although the primitives pass alone (tools/waitvalue_probe.hip) --
// with GPU_MAX_HW_QUEUES = 4 two streams can share one hardware queue, and a
// wait ahead of its own release in that queue never passes.  So a join blocks
// the calling thread until the worker has queued its last command, and calls
// started back to back (e.g. slices of a batch) run side by side
// (profiles/repair_async_r04.log).
int dagpu_repair_start(dagpu_ctx* ctx, uint32_t k, size_t n, uint8_t* d_eds, uint8_t* d_present,
                       const uint8_t* d_row_roots, const uint8_t* d_col_roots, int32_t* d_status,
                       void* d_workspace, void* stream, uint64_t* handle) {
  if (!ctx || !handle || !d_eds || !d_present || !d_row_roots || !d_col_roots || !d_status || !d_workspace)
    return DAGPU_ERR_ARG;
  *handle = 0;
  int rc = check_k(ctx, k);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  std::lock_guard<std::mutex> g(ctx->async_mu);
  int si = -1;
  for (int i = 0; i < dagpu_ctx::kAsyncSlots && si < 0; i++)
    if (!ctx->async_slot[i].busy) si = i;
  if (si < 0) return set_err(ctx, DAGPU_ERR_ARG, "too many repairs started and not joined");
  dagpu_ctx::AsyncSlot& sl = ctx->async_slot[si];
  HIP_TRY(ctx, async_init_slot(sl));
  HIP_TRY(ctx, launch_rs_prepare((int)k));  // first-use table uploads here, not on the worker
  HIP_TRY(ctx, hipEventRecord(sl.fork, s));
  sl.rc = DAGPU_OK;
  sl.err.clear();
  for (auto& x : sl.stats) x = 0;
  hipStream_t ws = sl.stream;
  hipEvent_t fork = sl.fork, fin = sl.finished;
  dagpu_ctx::AsyncSlot* slp = &sl;
  const int dev = ctx->device;
  // std::thread / make_shared may throw (no threads or memory left): nothing
  // may escape an extern "C" entry point, and the slot stays free
  try {
    auto mb = std::make_shared<Mailbox>(ctx);
    auto snap = std::make_shared<SwSnapshot>();
    sw_snapshot(snap.get());  // on the caller's thread (getenv is not thread-safe against setenv)
#ifdef DAGPU_TEST_HOOKS
    const char* inj = getenv("DAGPU_TEST_WORKER_FAIL");
    const bool inject_fail = inj && inj[0] == '1';
#endif
    sl.worker = std::thread([=]() {
      on_repair_worker() = true;
      sw_bind(snap.get());  // the switches as the start call saw them
      (void)hipSetDevice(dev);
      int r = hipStreamWaitEvent(ws, fork, 0) == hipSuccess ? DAGPU_OK : DAGPU_ERR_DEVICE;
#ifdef DAGPU_TEST_HOOKS
      // test build only (libdagpu_test.so, tests/test_gpu_repair_async.py): the
      // worker fails before its first kernel, so the join's error path is exercised
      if (r == DAGPU_OK && inject_fail) r = set_err(ctx, DAGPU_ERR_DEVICE, "injected worker failure");
#endif
      if (r == DAGPU_OK && n)
        r = repair_device(ctx, k, n, d_eds, d_present, d_row_roots, d_col_roots, d_status, nullptr, d_workspace, ws,
                          mb.get(), slp->stats);
      if (r != DAGPU_OK) {
        // the worker's own message (set_err wrote it to this thread's state);
        // the join re-raises it on the caller's thread
        const ThreadErr& te = thread_err();
        slp->err = te.own && !te.msg.empty() ? te.msg : "started repair failed on the device";
        (void)hipMemsetD32Async((hipDeviceptr_t)d_status, (int)DAGPU_ERR_DEVICE, n, ws);
      }
      (void)hipEventRecord(fin, ws);
      slp->rc = r;
    });
  } catch (...) {
    return set_err(ctx, DAGPU_ERR_DEVICE, "could not start the repair worker thread");
  }
  if (++ctx->async_gen == 0) ++ctx->async_gen;
  sl.busy = true;
  sl.joining = false;
  sl.gen = ctx->async_gen;
  *handle = ((uint64_t)sl.gen << 8) | (uint64_t)si;
  return DAGPU_OK;
}

int dagpu_repair_join(dagpu_ctx* ctx, uint64_t handle, void* stream) {
  if (!ctx) return DAGPU_ERR_ARG;
  const int si = (int)(handle & 0xFF);
  std::thread worker;
  {  // claim the slot under the lock, wait for its worker without it
    std::lock_guard<std::mutex> g(ctx->async_mu);
    if (si >= dagpu_ctx::kAsyncSlots || !ctx->async_slot[si].busy || ctx->async_slot[si].joining ||
        ctx->async_slot[si].gen != (uint32_t)(handle >> 8))
      return set_err(ctx, DAGPU_ERR_ARG, "unknown or already joined repair handle");
    ctx->async_slot[si].joining = true;
    worker = std::move(ctx->async_slot[si].worker);
  }
  if (worker.joinable()) worker.join();  // its last command is queued
  std::lock_guard<std::mutex> g(ctx->async_mu);
  dagpu_ctx::AsyncSlot& sl = ctx->async_slot[si];
  const int rc = sl.rc;
  {
    std::lock_guard<std::mutex> gp(ctx->prof_mu);
    for (int i = 0; i < DAGPU_REPAIR_STATS; i++) ctx->rep_stats[i] = sl.stats[i];
  }
  const hipError_t e = hipStreamWaitEvent((hipStream_t)stream, sl.finished, 0);
  sl.busy = false;
  sl.joining = false;
  if (e != hipSuccess) return hip_fail(ctx, e, "hipStreamWaitEvent(stream, finished)");
  if (rc != DAGPU_OK) return set_err(ctx, rc, sl.err);
  return DAGPU_OK;
}

// Start + join on the same stream: returns once every kernel of the repair is
// queued (the caller's stream then runs them in order with its later work).
int dagpu_repair_batch_device(dagpu_ctx* ctx, uint32_t k, size_t n, uint8_t* d_eds,
                              uint8_t* d_present, const uint8_t* d_row_roots,
                              const uint8_t* d_col_roots, int32_t* d_status, void* d_workspace,
                              void* stream) {
  if (!ctx || !d_eds || !d_present || !d_row_roots || !d_col_roots || !d_status || !d_workspace)
    return DAGPU_ERR_ARG;
  int rc = check_k(ctx, k);
  if (rc) return rc;
  if (n == 0) return DAGPU_OK;
  return repair_device(ctx, k, n, d_eds, d_present, d_row_roots, d_col_roots, d_status, nullptr, d_workspace,
                       (hipStream_t)stream);
}

int dagpu_repair_ex(dagpu_ctx* ctx, uint32_t k, uint8_t* eds, uint8_t* present,
                    const uint8_t* row_roots, const uint8_t* col_roots, int32_t* byz) {
  if (!ctx || !eds || !present || !row_roots || !col_roots) return DAGPU_ERR_ARG;
  std::lock_guard<std::mutex> g(ctx->mu);
  (void)hipSetDevice(ctx->device);
  if (byz) byz[0] = byz[1] = byz[2] = byz[3] = -1;
  int rc = check_k(ctx, k);
  if (rc) return rc;
  const size_t w = 2 * (size_t)k;
  hipStream_t s = ctx->stream;
  HIP_TRY(ctx, ctx->eds.ensure(eds_bytes(k)));
  HIP_TRY(ctx, ctx->ods.ensure(w * w));
  HIP_TRY(ctx, ctx->rr.ensure(w * kNodeSize));
  HIP_TRY(ctx, ctx->cr.ensure(w * kNodeSize));
  HIP_TRY(ctx, ctx->status.ensure(5 * sizeof(int32_t)));
  HIP_TRY(ctx, ctx->ws.ensure(dagpu_repair_workspace_size(k, 1)));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->eds.p, eds, eds_bytes(k), hipMemcpyHostToDevice, s));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->ods.p, present, w * w, hipMemcpyHostToDevice, s));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->rr.p, row_roots, w * kNodeSize, hipMemcpyHostToDevice, s));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->cr.p, col_roots, w * kNodeSize, hipMemcpyHostToDevice, s));
  int32_t* d_st = (int32_t*)ctx->status.p;
  rc = repair_device(ctx, k, 1, (uint8_t*)ctx->eds.p, (uint8_t*)ctx->ods.p, (const uint8_t*)ctx->rr.p,
                     (const uint8_t*)ctx->cr.p, d_st, d_st + 1, ctx->ws.p, s);
  if (rc) return rc;
  int32_t st[5] = {0, -1, -1, -1, -1};
  HIP_TRY(ctx, hipMemcpyAsync(st, d_st, sizeof st, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipMemcpyAsync(eds, ctx->eds.p, eds_bytes(k), hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipMemcpyAsync(present, ctx->ods.p, w * w, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  if (byz) memcpy(byz, st + 1, 4 * sizeof(int32_t));
  const char* axn = st[1] == 1 ? "col" : "row";
  switch (st[0]) {
    case DAGPU_OK: return DAGPU_OK;
    case DAGPU_ERR_BAD_ROOTS: {
      // "bad root input: row %d expected %v got %v" (prerepairSanityCheck)
      const RepairWs r = carve_repair(k, 1, ctx->ws.p);
      std::vector<uint8_t> got(kNodeSize);
      const uint8_t* src = (st[1] == 1 ? r.sa.col_roots : r.sa.row_roots) + (size_t)st[2] * kNodeSize;
      HIP_TRY(ctx, hipMemcpy(got.data(), src, kNodeSize, hipMemcpyDeviceToHost));
      const uint8_t* want = (st[1] == 1 ? col_roots : row_roots) + (size_t)st[2] * kNodeSize;
      return set_err(ctx, st[0], std::string("bad root input: ") + axn + " " + std::to_string(st[2]) +
                                     " expected " + go_bytes(want, kNodeSize) + " got " +
                                     go_bytes(got.data(), kNodeSize));
    }
    case DAGPU_ERR_BYZANTINE:  // ErrByzantineData.Error(): "byzantine %s: %d"
      return set_err(ctx, st[0], st[1] >= 0 ? std::string("byzantine ") + axn + ": " + std::to_string(st[2])
                                            : std::string("byzantine data"));
    case DAGPU_ERR_UNREPAIRABLE: return set_err(ctx, st[0], "failed to solve data square");
    default: return set_err(ctx, st[0], "repair failed");
  }
}

int dagpu_repair(dagpu_ctx* ctx, uint32_t k, uint8_t* eds, uint8_t* present,
                 const uint8_t* row_roots, const uint8_t* col_roots) {
  return dagpu_repair_ex(ctx, k, eds, present, row_roots, col_roots, nullptr);
}

int dagpu_repair_stats(dagpu_ctx* ctx, int64_t* out) {
  if (!ctx || !out) return DAGPU_ERR_ARG;
  std::lock_guard<std::mutex> g(ctx->prof_mu);
  for (int i = 0; i < DAGPU_REPAIR_STATS; i++) out[i] = ctx->rep_stats[i];
  return DAGPU_OK;
}

}  // extern "C"
