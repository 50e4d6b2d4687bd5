// dagpu.cpp -- C-ABI host runtime for the MI355X DA hot path (include/dagpu.h).
//
// Mirrors the reference entry points:
//   da.ExtendShares            pkg/da/data_availability_header.go:65-75
//   da.NewDataAvailabilityHeader / Hash   :44-63, :92-108
//   rsmt2d.ComputeExtendedDataSquare (3k Encode calls) via the Leopard codec
//   appconsts.DefaultCodec     pkg/appconsts/global_consts.go:92
// The pipeline per batch of same-k squares (all on one HIP stream):
//   row encode Q0 -> Q1 (+ Q0 placement)  |  column encode [Q0|Q1] -> [Q2|Q3]
//   leaf digests (each cell once)  |  row+col NMT trees  |  DAH
// The EDS never leaves HBM unless the caller asks for it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/dagpu.h"
#include "host_sha256.hpp"
#include "kernels.hpp"
#include "pipe_carve.hpp"
#include "runtime.hpp"

using namespace dagpu;

namespace dagpu {

// d_dah = NULL: roots only (Repair's verification needs no DAH).  The leaf
// launch clears the status words (no memset in front of it).
int enqueue_roots(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* d_eds, uint8_t* d_rr,
                  uint8_t* d_cr, uint8_t* d_dah, int32_t* d_status, void* d_ws, hipStream_t s) {
  SquareArgs sa{};
  sa.eds = d_eds;
  sa.eds_sq_stride = (long)eds_bytes(k);
  sa.k = (int)k;
  sa.nsq = (long)n;
  nmt_workspace_carve(sa, d_ws);
  sa.row_roots = d_rr;
  sa.col_roots = d_cr;
  sa.dah = d_dah;
  sa.status = d_status;
  sa.k = (int)k;
  sa.nsq = (long)n;
  {
    ProfScope p(ctx, 2, s);
    HIP_TRY(ctx, launch_nmt_leaves(sa, s, 0, -1, true));
  }
  stage_mark(ctx, DAGPU_STAGE_LEAVES, s);
  {
    ProfScope p(ctx, 3, s);
    HIP_TRY(ctx, launch_nmt_trees(sa, s));
  }
  stage_mark(ctx, DAGPU_STAGE_TREES, s);
  if (d_dah) {
    ProfScope p(ctx, 4, s);
    HIP_TRY(ctx, launch_dah(sa, s));
  }
  stage_mark(ctx, DAGPU_STAGE_DAH, s);
  return DAGPU_OK;
}

// Completion wait of a host-path call.  Calls that finish in about a
// millisecond (single squares, the production callers' shape) spin on the
// stream: the blocking wait's wake-up added up to 0.25 ms to single-square
// calls (bench.py single_square stages, r03).
hipError_t wait_stream(hipStream_t s, bool spin) {
  if (!spin) return hipStreamSynchronize(s);
  hipError_t e;
  while ((e = hipStreamQuery(s)) == hipErrorNotReady) __builtin_ia32_pause();
  return e;
}

}  // namespace dagpu

namespace {

// RS extension of n squares (uniform k), device pointers.
// ev_rows (optional) is recorded between the row and the column pass: rows
// 0..k-1 of every EDS ([Q0|Q1]) are final from that point on (the host path
// starts the EDS download there, the sliced device batch the top-half leaves).
int enqueue_rs(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* d_ods, uint8_t* d_eds,
               hipStream_t s, hipEvent_t ev_rows = nullptr) {
  // Row pass: vector r = row r of Q0 -> Q1 (and copy Q0 into place); the rows
  // of [Q2|Q3] do not exist yet.
  EncodeArgs ra = axis_encode_args(k, n, d_eds, 0);
  ra.nvec = k;
  if (d_ods) {
    ra.in = d_ods;
    ra.in_sq_stride = (long)ods_bytes(k);
    ra.in_vec_stride = (long)k * kSS;
    ra.copy = d_eds;
    ra.copy_sq_stride = (long)eds_bytes(k);
    ra.copy_vec_stride = 2L * k * kSS;
    ra.copy_shard_stride = kSS;
  }
  {
    ProfScope p(ctx, 0, s);
    HIP_TRY(ctx, launch_rs_encode((int)k, ra, s));
  }
  stage_mark(ctx, DAGPU_STAGE_ROWS, s);
  if (ev_rows) HIP_TRY(ctx, hipEventRecord(ev_rows, s));
  // Column pass: vector c = column c of [Q0|Q1] -> [Q2|Q3].
  const EncodeArgs ca = axis_encode_args(k, n, d_eds, 1);
  {
    ProfScope p(ctx, 1, s);
    HIP_TRY(ctx, launch_rs_encode((int)k, ca, s));
  }
  stage_mark(ctx, DAGPU_STAGE_COLS, s);
  return DAGPU_OK;
}

// Events of one pipelined call, back in the pool on every return path.
struct EventSet {
  dagpu_ctx* c;
  std::vector<hipEvent_t> v;
  explicit EventSet(dagpu_ctx* ctx) : c(ctx) {}
  ~EventSet() {
    for (auto e : v) ev_give(c, e);
  }
  bool take(size_t n) {
    for (size_t i = 0; i < n; i++) {
      hipEvent_t e = ev_take(c);
      if (!e) return false;
      v.push_back(e);
    }
    return true;
  }
};

// dagpu_extend_batch_device with S >= 2 slices.  The RS passes of all slices
// run in order on a side stream; the caller's stream hashes slice after slice:
//   top-half leaves (rows 0..k-1: final after the slice's ROW pass, so they
//   run beside its column pass; they also clear the slice's status words)
//   |  bottom-half leaves (after the column pass)  |  tree levels 1..cut
// and then, once over all n squares, tree levels cut+1.. and the DAH: at a
// slice's size those launches cannot fill the CUs (pipe_carve.hpp has the rule
// for `cut` and the workspace layout).  Profiling never comes here
// (pipe_slices), so no launch is bracketed.
int extend_batch_sliced(dagpu_ctx* ctx, uint32_t k, size_t n, size_t S, const uint8_t* d_ods, uint8_t* d_eds,
                        uint8_t* d_rr, uint8_t* d_cr, uint8_t* d_dah, int32_t* d_status, void* d_ws,
                        hipStream_t s) {
  const size_t w = 2 * (size_t)k;
  // equal slices (tried and dropped, profiles/pipeline_r02.log, pipe_streams_r03.log, pipe_tails_after.log:
  // a smaller first slice, a high-priority RS stream, a second NMT stream)
  std::vector<size_t> cut(S + 1);
  for (size_t i = 0; i <= S; i++) cut[i] = n * i / S;
  const size_t m = (n + S - 1) / S;  // the largest slice
  const int levels = nmt_levels((int)k);
  // the rule's cut level, or the next one whose batch-wide records still fit in
  // the caller's workspace (two slices at a low cut do not); none: every slice
  // runs all its levels in the unsliced layout
  PipeCarve pc{};
  for (int cl = pipe_cut_level((int)k, m, nmt_level_fill_blocks()); cl < levels && !pc.defer; cl++)
    pc = pipe_carve((int)k, n, m, cl, dagpu_workspace_size(k, n));
  // events: [0, S) a slice's RS done, [S, 2S) its row pass done, [2S] the fork
  EventSet ev(ctx);
  if (!ev.take(2 * S + 1)) return set_err(ctx, DAGPU_ERR_DEVICE, "hipEventCreate failed");
  hipStream_t rs = side_stream(ctx, s, 0);
  if (!rs) return set_err(ctx, DAGPU_ERR_DEVICE, "hipStreamCreate failed");
  // fork: the side stream starts after the work already queued on the caller's stream
  HIP_TRY(ctx, hipEventRecord(ev.v[2 * S], s));
  HIP_TRY(ctx, hipStreamWaitEvent(rs, ev.v[2 * S], 0));
  for (size_t i = 0; i < S; i++) {
    const size_t a = cut[i], b = cut[i + 1];
    int rc = enqueue_rs(ctx, k, b - a, d_ods ? d_ods + a * ods_bytes(k) : nullptr, d_eds + a * eds_bytes(k), rs,
                        ev.v[S + i]);
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(ev.v[i], rs));
  }
  uint8_t* const ws = (uint8_t*)d_ws;
  SquareArgs all{};  // the whole batch: deferred tree levels and the DAH
  all.eds = d_eds;
  all.eds_sq_stride = (long)eds_bytes(k);
  all.k = (int)k;
  all.nsq = (long)n;
  all.digests = ws;  // scratch of the DAH's two-stage variant, free once the trees are built
  all.ns_table = pc.defer ? ws + pc.ns_all : nullptr;
  all.row_roots = d_rr;
  all.col_roots = d_cr;
  all.dah = d_dah;
  all.status = d_status;
  // slices in order on the caller's stream, sharing the slice regions of the
  // workspace; waiting on the last slice's event joins the RS stream
  for (size_t i = 0; i < S; i++) {
    const size_t a = cut[i], b = cut[i + 1];
    SquareArgs sa = all;
    sa.eds = d_eds + a * eds_bytes(k);
    sa.nsq = (long)(b - a);
    sa.row_roots = d_rr + a * w * kNodeSize;
    sa.col_roots = d_cr + a * w * kNodeSize;
    sa.status = d_status + a;
    if (pc.defer) {
      sa.digests = ws + pc.digests;
      sa.rec_a = ws + pc.rec_a;
      sa.rec_b = ws + pc.rec_b;
      sa.ns_table = ws + pc.ns_all + a * (size_t)k * k * 32;
    } else {
      nmt_workspace_carve(sa, ws);
    }
    HIP_TRY(ctx, hipStreamWaitEvent(s, ev.v[S + i], 0));
    HIP_TRY(ctx, launch_nmt_leaves(sa, s, 0, (int)k, true));
    HIP_TRY(ctx, hipStreamWaitEvent(s, ev.v[i], 0));
    HIP_TRY(ctx, launch_nmt_leaves(sa, s, (int)k, (int)k, false));
    uint8_t* const pp[2] = {sa.rec_b, sa.rec_a};
    uint8_t* const cut_out = pc.defer ? ws + pc.rec_c + a * nmt_level_rec_bytes((int)k, pc.cut) : nullptr;
    HIP_TRY(ctx, launch_nmt_tree_levels(sa, 1, pc.defer ? pc.cut : levels, pp, cut_out, s));
  }
  if (pc.defer) {
    uint8_t* const pp[2] = {ws + pc.rec_c, ws + pc.rec_d};
    HIP_TRY(ctx, launch_nmt_tree_levels(all, pc.cut + 1, levels, pp, nullptr, s));
  }
  HIP_TRY(ctx, launch_dah(all, s));
  return DAGPU_OK;
}

// Squares per pipeline chunk: about 128 MiB of ODS per host->device copy.
// DAGPU_PIPELINE_CHUNK (squares) overrides it, e.g. to exercise many chunks in tests.
size_t pipeline_chunk(uint32_t k, size_t n) {
  size_t m = (size_t(128) << 20) / ods_bytes(k);
  const long v = sw_long(SW_PIPELINE_CHUNK);
  if (v > 0) m = (size_t)v;
  return m < 1 ? 1 : (m > n ? n : m);
}

int finish_status(dagpu_ctx* ctx, const int32_t* st, size_t n, int32_t* status) {
  int first = DAGPU_OK;
  for (size_t i = 0; i < n; i++) {
    int v = (st[i] & kStatusPushOrder) ? DAGPU_ERR_PUSH_ORDER : DAGPU_OK;
    if (status) status[i] = v;
    if (v && !first) first = v;
  }
  if (first) set_err(ctx, first, "invalid push order: namespaces of original data square are not sorted");
  return first;
}

// Host-mode batch of >= 2 chunks: chunk c's ODS goes up on copy_stream while
// chunk c-1 is extended on ctx->stream; roots, DAHs and status come back into
// page-locked staging per slot and are copied to the caller's arrays once the
// slot's event fires (the caller's buffers may be pageable Go memory, whose
// device->host copies would otherwise block this thread and the pipeline).
// An EDS requested back is copied straight into eds_out.  Caller holds ctx->mu.
int run_group_pipelined(dagpu_ctx* ctx, uint32_t k, size_t n, size_t m, const uint8_t* ods,
                        uint8_t* eds_out, uint8_t* rr, uint8_t* cr, uint8_t* dah, int32_t* status) {
  const size_t w = 2 * (size_t)k;
  const size_t rb = w * kNodeSize, ob = ods_bytes(k), eb = eds_bytes(k);
  const size_t wsb = dagpu_workspace_size(k, m);
  hipStream_t s = ctx->stream, cs = ctx->copy_stream;
  HIP_TRY(ctx, ctx->ods.ensure(2 * m * ob));
  HIP_TRY(ctx, ctx->eds.ensure(2 * m * eb));
  HIP_TRY(ctx, ctx->rr.ensure(2 * m * rb));
  HIP_TRY(ctx, ctx->cr.ensure(2 * m * rb));
  HIP_TRY(ctx, ctx->dah.ensure(2 * m * 32));
  HIP_TRY(ctx, ctx->status.ensure(2 * m * sizeof(int32_t)));
  HIP_TRY(ctx, ctx->ws.ensure(2 * wsb));
  const size_t hslot = m * (2 * rb + 32 + sizeof(int32_t));
  HIP_TRY(ctx, ctx->h_out.ensure(2 * hslot));
  std::vector<int32_t> st(n);
  const size_t nchunks = (n + m - 1) / m;
  auto slot_dev = [&](DevBuf& b, size_t per, int slot) { return (uint8_t*)b.p + slot * m * per; };
  auto slot_host = [&](int slot) { return (uint8_t*)ctx->h_out.p + slot * hslot; };
  // copy chunk c's outputs from its slot's staging to the caller (slot's event done)
  auto drain = [&](size_t c) -> int {
    const int slot = (int)(c & 1);
    const size_t off = c * m, cnt = (n - off < m) ? n - off : m;
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev_done[slot]));
    const uint8_t* h = slot_host(slot);
    memcpy(rr + off * rb, h, cnt * rb);
    memcpy(cr + off * rb, h + m * rb, cnt * rb);
    memcpy(dah + off * 32, h + 2 * m * rb, cnt * 32);
    memcpy(st.data() + off, h + 2 * m * rb + m * 32, cnt * sizeof(int32_t));
    return DAGPU_OK;
  };
  for (size_t c = 0; c < nchunks; c++) {
    const int slot = (int)(c & 1);
    const size_t off = c * m, cnt = (n - off < m) ? n - off : m;
    if (c >= 2) {  // the slot's previous chunk must be drained before reuse
      int rc = drain(c - 2);
      if (rc) return rc;
      HIP_TRY(ctx, hipStreamWaitEvent(cs, ctx->ev_done[slot], 0));
    }
    uint8_t* d_ods = slot_dev(ctx->ods, ob, slot);
    uint8_t* d_eds = slot_dev(ctx->eds, eb, slot);
    uint8_t* d_rr = slot_dev(ctx->rr, rb, slot);
    uint8_t* d_cr = slot_dev(ctx->cr, rb, slot);
    uint8_t* d_dah = slot_dev(ctx->dah, 32, slot);
    int32_t* d_st = (int32_t*)slot_dev(ctx->status, sizeof(int32_t), slot);
    HIP_TRY(ctx, hipMemcpyAsync(d_ods, ods + off * ob, cnt * ob, hipMemcpyHostToDevice, cs));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_loaded[slot], cs));
    HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->ev_loaded[slot], 0));
    int rc = enqueue_rs(ctx, k, cnt, d_ods, d_eds, s);
    if (rc) return rc;
    rc = enqueue_roots(ctx, k, cnt, d_eds, d_rr, d_cr, d_dah, d_st, (uint8_t*)ctx->ws.p + slot * wsb, s);
    if (rc) return rc;
    if (eds_out)
      HIP_TRY(ctx, hipMemcpyAsync(eds_out + off * eb, d_eds, cnt * eb, hipMemcpyDeviceToHost, s));
    uint8_t* h = slot_host(slot);
    HIP_TRY(ctx, hipMemcpyAsync(h, d_rr, cnt * rb, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(h + m * rb, d_cr, cnt * rb, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(h + 2 * m * rb, d_dah, cnt * 32, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(h + 2 * m * rb + m * 32, d_st, cnt * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_done[slot], s));
  }
  for (size_t c = nchunks >= 2 ? nchunks - 2 : 0; c < nchunks; c++) {
    int rc = drain(c);
    if (rc) return rc;
  }
  return finish_status(ctx, st.data(), n, status);
}

// Roots, DAHs and status of a host-path call share one device buffer
// (ctx->res: rr | cr | dah | status) and come back in ONE copy to page-locked
// staging, then go to the caller's (possibly pageable) arrays by memcpy: four
// small device->host copies cost ~20 us each on the single-square latency path
// (profiles/single_square_r02.log).  Caller holds ctx->mu.
struct HostResults {
  size_t n = 0, rb = 0, bytes = 0;
  uint8_t *rr = nullptr, *cr = nullptr, *dah = nullptr;
  int32_t* st = nullptr;
  hipError_t alloc(dagpu_ctx* ctx, uint32_t k, size_t cnt) {
    n = cnt;
    rb = 2 * (size_t)k * kNodeSize * n;
    bytes = 2 * rb + 32 * n + sizeof(int32_t) * n;
    hipError_t e = ctx->res.ensure(bytes);
    if (e == hipSuccess) e = ctx->h_out.ensure(bytes);
    if (e != hipSuccess) return e;
    rr = (uint8_t*)ctx->res.p;
    cr = rr + rb;
    dah = cr + rb;
    st = (int32_t*)(dah + 32 * n);  // rb = 180 k n: 4-byte aligned
    return hipSuccess;
  }
  hipError_t download(dagpu_ctx* ctx, hipStream_t s) const {
    return hipMemcpyAsync(ctx->h_out.p, ctx->res.p, bytes, hipMemcpyDeviceToHost, s);
  }
  // after the stream has synchronised
  void deliver(const dagpu_ctx* ctx, uint8_t* o_rr, uint8_t* o_cr, uint8_t* o_dah, int32_t* o_st) const {
    const uint8_t* h = (const uint8_t*)ctx->h_out.p;
    memcpy(o_rr, h, rb);
    memcpy(o_cr, h + rb, rb);
    memcpy(o_dah, h + 2 * rb, 32 * n);
    memcpy(o_st, h + 2 * rb + 32 * n, sizeof(int32_t) * n);
  }
};

// hipHostMalloc / hipHostRegister memory: device->host copies into it are
// asynchronous DMA.  Into pageable memory they run synchronously on this thread.
bool host_pinned(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeHost;
}

// Runs one uniform-k group from host memory.  Caller holds ctx->mu.
int run_group_host(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* ods, uint8_t* eds_out,
                   uint8_t* rr, uint8_t* cr, uint8_t* dah, int32_t* status) {
  int rc = check_k(ctx, k);
  if (rc) return rc;
  const size_t m = pipeline_chunk(k, n);
  if (n > m) return run_group_pipelined(ctx, k, n, m, ods, eds_out, rr, cr, dah, status);
  hipStream_t s = ctx->stream, cs = ctx->copy_stream;
  const bool spin = eds_bytes(k) * n <= (size_t(64) << 20);
  HostResults res;
  HIP_TRY(ctx, ctx->ods.ensure(ods_bytes(k) * n));
  HIP_TRY(ctx, ctx->eds.ensure(eds_bytes(k) * n));
  HIP_TRY(ctx, res.alloc(ctx, k, n));
  HIP_TRY(ctx, ctx->ws.ensure(dagpu_workspace_size(k, n)));
  ctx->stage_mask = 0;
  stage_mark(ctx, DAGPU_STAGE_START, s);
  HIP_TRY(ctx, hipMemcpyAsync(ctx->ods.p, ods, ods_bytes(k) * n, hipMemcpyHostToDevice, s));
  stage_mark(ctx, DAGPU_STAGE_UPLOADED, s);
  // An EDS requested back goes down on the copy stream while the kernels run:
  // the top halves ([Q0|Q1], final after the row pass) during the column pass
  // and the NMT kernels, the bottom halves ([Q2|Q3]) during the NMT kernels.
  // Into page-locked memory the copies are queued right after the RS passes,
  // so the DMA starts as soon as the rows are final.  Into pageable memory a
  // device->host copy runs synchronously on this thread, so there the whole
  // kernel chain and the results download are queued first.
  rc = enqueue_rs(ctx, k, n, (const uint8_t*)ctx->ods.p, (uint8_t*)ctx->eds.p, s,
                  eds_out ? ctx->ev_loaded[0] : nullptr);
  if (rc) return rc;
  if (eds_out) HIP_TRY(ctx, hipEventRecord(ctx->ev_loaded[1], s));
  // from the first EDS copy on, DMA may be writing into eds_out: every return
  // path waits for the copy stream
  struct CopyJoin {
    hipStream_t cs;
    bool armed = false;
    ~CopyJoin() {
      if (armed) (void)hipStreamSynchronize(cs);
    }
  } join{cs};
  auto eds_copies = [&]() -> int {
    join.armed = true;
    const size_t eb = eds_bytes(k), half = eb / 2;
    HIP_TRY(ctx, hipStreamWaitEvent(cs, ctx->ev_loaded[0], 0));
    const uint8_t* d = (const uint8_t*)ctx->eds.p;
    for (size_t i = 0; i < n; i++)  // plain 1D copies: the DMA engines' fast path
      HIP_TRY(ctx, hipMemcpyAsync(eds_out + i * eb, d + i * eb, half, hipMemcpyDeviceToHost, cs));
    stage_mark(ctx, DAGPU_STAGE_EDS_TOP, cs);
    HIP_TRY(ctx, hipStreamWaitEvent(cs, ctx->ev_loaded[1], 0));
    for (size_t i = 0; i < n; i++)
      HIP_TRY(ctx, hipMemcpyAsync(eds_out + i * eb + half, d + i * eb + half, half,
                                  hipMemcpyDeviceToHost, cs));
    stage_mark(ctx, DAGPU_STAGE_EDS_BOTTOM, cs);
    return DAGPU_OK;
  };
  const bool early = eds_out && host_pinned(eds_out);
  if (early && (rc = eds_copies())) return rc;
  rc = enqueue_roots(ctx, k, n, (const uint8_t*)ctx->eds.p, res.rr, res.cr, res.dah, res.st, ctx->ws.p, s);
  if (rc) return rc;
  HIP_TRY(ctx, res.download(ctx, s));
  stage_mark(ctx, DAGPU_STAGE_RESULTS, s);
  if (eds_out && !early && (rc = eds_copies())) return rc;
  if (eds_out) {
    HIP_TRY(ctx, wait_stream(cs, spin));
    join.armed = false;
  }
  HIP_TRY(ctx, wait_stream(s, spin));
  std::vector<int32_t> st(n);
  res.deliver(ctx, rr, cr, dah, st.data());
  return finish_status(ctx, st.data(), n, status);
}

}  // namespace

extern "C" {

int dagpu_version(void) { return 100; }

uint32_t dagpu_max_square_width(void) {
  static_assert(DAGPU_MAX_SQUARE_WIDTH == kMaxK, "header and kernels disagree on the widest square");
  return (uint32_t)kMaxK;
}

uint32_t dagpu_max_codec_width(void) {
  static_assert(DAGPU_MAX_CODEC_WIDTH == kMaxCodecK, "header and kernels disagree on the widest codec vector");
  return (uint32_t)kMaxCodecK;
}

int dagpu_init(int device, dagpu_ctx** out) {
  if (!out) return DAGPU_ERR_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return DAGPU_ERR_DEVICE;
  if (device < 0 || device >= ndev) return DAGPU_ERR_ARG;
  if (hipSetDevice(device) != hipSuccess) return DAGPU_ERR_DEVICE;
  dagpu_ctx* c = new dagpu_ctx();
  c->device = device;
  c->gen = next_ctx_gen();
  bool ok = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess &&
            hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) == hipSuccess;
  for (int i = 0; ok && i < 2; i++)
    ok = hipEventCreateWithFlags(&c->ev_loaded[i], hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&c->ev_done[i], hipEventDisableTiming) == hipSuccess;
  for (int i = 0; ok && i < dagpu_ctx::kStages; i++) ok = hipEventCreate(&c->stage_ev[i]) == hipSuccess;
  if (!ok) {
    dagpu_destroy(c);
    return DAGPU_ERR_DEVICE;
  }
  *out = c;
  return DAGPU_OK;
}

void dagpu_destroy(dagpu_ctx* c) {
  if (!c) return;
  if (thread_err().ctx == c && thread_err().gen == c->gen) thread_err() = ThreadErr{};
  (void)hipSetDevice(c->device);
  for (auto& sl : c->async_slot) {  // started Repairs finish first
    if (sl.worker.joinable()) sl.worker.join();
    if (sl.stream) (void)hipStreamSynchronize(sl.stream);
  }
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
  c->h_out.release();
  c->commit_stage.release();
  c->res.release();
  c->ods.release(); c->eds.release(); c->rr.release(); c->cr.release();
  c->dah.release(); c->status.release(); c->ws.release();
  for (DevBuf* b : {&c->t_leaf_data, &c->t_leaves, &c->t_inner, &c->t_meta, &c->t_out, &c->t_status, &c->t_flags})
    b->release();
  for (auto& r : c->pending) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  for (auto e : c->pool) (void)hipEventDestroy(e);
  for (int i = 0; i < 2; i++) {
    if (c->ev_loaded[i]) (void)hipEventDestroy(c->ev_loaded[i]);
    if (c->ev_done[i]) (void)hipEventDestroy(c->ev_done[i]);
  }
  for (auto e : c->stage_ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& cs : c->side)
    for (hipStream_t x : {cs.rs, cs.rs_hi})
      if (x) (void)hipStreamSynchronize(x);
  for (auto e : c->ev_pool) (void)hipEventDestroy(e);
  for (void* m : c->mailboxes) (void)hipHostFree(m);
  for (auto& cs : c->side)
    for (hipStream_t x : {cs.rs, cs.rs_hi})
      if (x) (void)hipStreamDestroy(x);
  for (auto& sl : c->async_slot) {
    if (sl.fork) (void)hipEventDestroy(sl.fork);
    if (sl.finished) (void)hipEventDestroy(sl.finished);
    if (sl.stream) (void)hipStreamDestroy(sl.stream);
  }
  if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

void* dagpu_host_alloc(size_t bytes) {
  void* p = nullptr;
  return hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess ? p : nullptr;
}

void dagpu_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

int dagpu_host_register(void* p, size_t bytes) {
  if (!p || !bytes) return DAGPU_ERR_ARG;
  return hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess ? DAGPU_OK : DAGPU_ERR_DEVICE;
}

int dagpu_host_unregister(void* p) {
  if (!p) return DAGPU_ERR_ARG;
  return hipHostUnregister(p) == hipSuccess ? DAGPU_OK : DAGPU_ERR_DEVICE;
}

// The message of this thread's last failure on `c`; if this thread has not
// failed on `c`, a snapshot of the context's most recent message.  The pointer
// stays valid until this thread's next call into the library.
const char* dagpu_last_error(dagpu_ctx* c) {
  ThreadErr& t = thread_err();
  if (!c) return t.ctx == nullptr && t.own ? t.msg.c_str() : "null context";
  if (t.ctx == c && t.gen == c->gen && t.own) return t.msg.c_str();
  std::lock_guard<std::mutex> g(c->err_mu);
  t.ctx = c;
  t.gen = c->gen;
  t.own = false;
  t.msg = c->err;
  return t.msg.c_str();
}

size_t dagpu_workspace_size(uint32_t k, size_t n) {
  if (k == 0 || n == 0) return 256;
  return nmt_workspace_bytes((int)k, (long)n) + 256;
}

int dagpu_extend_shares(dagpu_ctx* ctx, const uint8_t* shares, size_t n_shares,
                        size_t share_size, uint8_t* eds_out, uint8_t* row_roots,
                        uint8_t* col_roots, uint8_t* dah) {
  if (!ctx || !row_roots || !col_roots || !dah) return DAGPU_ERR_ARG;
  std::lock_guard<std::mutex> g(ctx->mu);
  (void)hipSetDevice(ctx->device);
  // pkg/da/data_availability_header.go:67-69
  if (!is_pow2(n_shares)) {
    return set_err(ctx, DAGPU_ERR_NOT_POW2,
                   "number of shares is not a power of 2: got " + std::to_string(n_shares));
  }
  // SquareSize (:205-207) then rsmt2d newDataSquare's square check
  const uint64_t k = (uint64_t)std::llround(std::ceil(std::sqrt((double)n_shares)));
  if (k * k != n_shares) return set_err(ctx, DAGPU_ERR_NOT_SQUARE, "number of chunks must be a square number");
  if (share_size != kSS) {
    return set_err(ctx, DAGPU_ERR_SHARE_SIZE,
                   "share size must be " + std::to_string(kSS) + " bytes (appconsts.ShareSize)");
  }
  if (!shares) return DAGPU_ERR_ARG;
  int32_t st = 0;
  return run_group_host(ctx, (uint32_t)k, 1, shares, eds_out, row_roots, col_roots, dah, &st);
}

int dagpu_extend_batch(dagpu_ctx* ctx, const uint8_t* ods, const uint32_t* k, size_t n,
                       uint8_t* eds_or_null, uint8_t* row_roots, uint8_t* col_roots,
                       uint8_t* dah, int32_t* status) {
  if (!ctx || (n && (!ods || !k || !row_roots || !col_roots || !dah))) return DAGPU_ERR_ARG;
  std::lock_guard<std::mutex> g(ctx->mu);
  (void)hipSetDevice(ctx->device);
  // per-square offsets in the packed arrays
  std::vector<size_t> o_ods(n), o_eds(n), o_root(n);
  size_t a = 0, b = 0, c = 0;
  for (size_t i = 0; i < n; i++) {
    int rc = check_k(ctx, k[i]);
    if (rc) {
      if (status) status[i] = rc;
      return rc;
    }
    o_ods[i] = a; o_eds[i] = b; o_root[i] = c;
    a += ods_bytes(k[i]); b += eds_bytes(k[i]); c += 2ull * k[i] * kNodeSize;
  }
  // group consecutive runs of equal k (block replay batches are mostly uniform)
  int first = DAGPU_OK;
  size_t i = 0;
  std::vector<int32_t> st;
  while (i < n) {
    size_t j = i;
    while (j < n && k[j] == k[i]) j++;
    st.assign(j - i, 0);
    int rc = run_group_host(ctx, k[i], j - i, ods + o_ods[i],
                            eds_or_null ? eds_or_null + o_eds[i] : nullptr,
                            row_roots + o_root[i], col_roots + o_root[i], dah + 32 * i, st.data());
    if (rc && rc != DAGPU_ERR_PUSH_ORDER) return rc;
    for (size_t t = i; t < j; t++) {
      if (status) status[t] = st[t - i];
      if (st[t - i] && !first) first = st[t - i];
    }
    i = j;
  }
  return first;
}

int dagpu_extend_rs_device(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* d_ods,
                           uint8_t* d_eds, void* stream) {
  if (!ctx || !d_eds) return DAGPU_ERR_ARG;
  int rc = check_k(ctx, k);
  if (rc) return rc;
  return enqueue_rs(ctx, k, n, d_ods, d_eds, (hipStream_t)stream);
}

int dagpu_roots_device(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* d_eds,
                       uint8_t* d_row_roots, uint8_t* d_col_roots, uint8_t* d_dah,
                       int32_t* d_status, void* d_workspace, void* stream) {
  if (!ctx || !d_eds || !d_row_roots || !d_col_roots || !d_dah || !d_status || !d_workspace)
    return DAGPU_ERR_ARG;
  int rc = check_k(ctx, k);
  if (rc) return rc;
  return enqueue_roots(ctx, k, n, d_eds, d_row_roots, d_col_roots, d_dah, d_status, d_workspace,
                       (hipStream_t)stream);
}

extern "C++" {  // external C++ helpers (runtime.hpp): split.cpp forks onto the side streams too
namespace dagpu {

// ---- switches (switches.hpp) ----
namespace {
const char* const kSwNames[SW_COUNT] = {
    "DAGPU_PIPELINE_CHUNK", "DAGPU_PIPE_SLICES", "DAGPU_REPAIR_FILL", "DAGPU_SPLIT_SQUARE", "DAGPU_SPLIT_OVERLAP",
    "DAGPU_DAH_SPLIT",      "DAGPU_DEC_SLICED",  "DAGPU_ENC_SLICED",  "DAGPU_ENC_SLICED2",  "DAGPU_GF16_WIDE"};
thread_local const SwSnapshot* tl_sw = nullptr;
}  // namespace

const char* sw(Switch s) {
  if (s < 0 || s >= SW_COUNT) return nullptr;
  if (tl_sw) return tl_sw->set[s] ? tl_sw->v[s] : nullptr;
  return getenv(kSwNames[s]);
}

long sw_long(Switch s, long dflt) {
  const char* e = sw(s);
  return e ? atol(e) : dflt;
}

void sw_snapshot(SwSnapshot* out) {
  for (int i = 0; i < SW_COUNT; i++) {
    const char* e = getenv(kSwNames[i]);
    out->set[i] = e != nullptr;
    out->v[i][0] = 0;
    if (e) snprintf(out->v[i], sizeof out->v[i], "%s", e);
  }
}

void sw_bind(const SwSnapshot* snap) { tl_sw = snap; }

hipEvent_t ev_take(dagpu_ctx* c) {
  std::lock_guard<std::mutex> g(c->ev_mu);
  if (!c->ev_pool.empty()) {
    hipEvent_t e = c->ev_pool.back();
    c->ev_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
  return e;
}

void ev_give(dagpu_ctx* c, hipEvent_t e) {
  if (!e) return;
  std::lock_guard<std::mutex> g(c->ev_mu);
  c->ev_pool.push_back(e);
}

// Slices of a device batch for the RS/NMT pipeline: RS of slice i+1.. runs on
// a side stream while the NMT kernels of slice i run on the caller's stream
// (bench: 256 squares at k = 128, 4 slices 11.98 -> 11.63 ms; tools/pipe_exp.py).
// 8 slices from 256 squares on: with the top tree levels and the DAH run once
// per call (extend_batch_sliced) a slice no longer pays its own tail, and 8
// beat 4 (profiles/pipe_tails_after.log; measured at 256 squares only, so
// smaller batches keep 4).
// DAGPU_PIPE_SLICES overrides (1 = off; read per call, so tests can vary it).
// Off while profiling, so that every kernel's event bracket times that kernel alone.
size_t pipe_slices(dagpu_ctx* ctx, uint32_t k, size_t n) {
  const long env = sw_long(SW_PIPE_SLICES);
  if (ctx->prof) return 1;
  size_t s = env > 0 ? (size_t)env : (k >= 128 && n >= 64 ? (n >= 256 ? 8 : 4) : 1);
  while (s > 1 && n / s < 8) s >>= 1;
  return s < 1 ? 1 : s;
}

// The side streams paired with caller stream `s` (created on first use).
// which: 0 = normal priority, 1 = the device's greatest stream priority.
hipStream_t side_stream(dagpu_ctx* ctx, hipStream_t s, int which) {
  std::lock_guard<std::mutex> g(ctx->side_mu);
  dagpu_ctx::Side* sd = nullptr;
  for (auto& p : ctx->side)
    if (p.caller == s) sd = &p;
  if (!sd) {
    if (ctx->side.size() >= dagpu_ctx::kMaxSideStreams) {
      // more caller streams than side streams: share them round-robin (the
      // callers then serialise their side work, results are unaffected)
      const size_t i = (size_t)((((uint64_t)(uintptr_t)s) * 0x9E3779B97F4A7C15ull) >> 32) % ctx->side.size();
      sd = &ctx->side[i];
    } else {
      ctx->side.emplace_back();
      sd = &ctx->side.back();
      sd->caller = s;
    }
  }
  hipStream_t* slot = which == 1 ? &sd->rs_hi : &sd->rs;
  if (!*slot) {
    hipError_t e;
    if (which == 1) {
      int lo = 0, hi = 0;
      (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
      e = hipStreamCreateWithPriority(slot, hipStreamNonBlocking, hi);
    } else {
      e = hipStreamCreateWithFlags(slot, hipStreamNonBlocking);
    }
    if (e != hipSuccess) {
      *slot = nullptr;
      return nullptr;
    }
  }
  return *slot;
}

}  // namespace dagpu
}  // extern "C++"

int dagpu_extend_batch_device(dagpu_ctx* ctx, uint32_t k, size_t n, const uint8_t* d_ods,
                              uint8_t* d_eds, uint8_t* d_row_roots, uint8_t* d_col_roots,
                              uint8_t* d_dah, int32_t* d_status, void* d_workspace,
                              void* stream) {
  if (!ctx || !d_eds || !d_row_roots || !d_col_roots || !d_dah || !d_status || !d_workspace)
    return DAGPU_ERR_ARG;
  int rc = check_k(ctx, k);
  if (rc) return rc;
  const size_t S = pipe_slices(ctx, k, n);
  hipStream_t s = (hipStream_t)stream;
  if (S <= 1) {
    rc = enqueue_rs(ctx, k, n, d_ods, d_eds, s);
    if (rc) return rc;
    return enqueue_roots(ctx, k, n, d_eds, d_row_roots, d_col_roots, d_dah, d_status, d_workspace, s);
  }
  return extend_batch_sliced(ctx, k, n, S, d_ods, d_eds, d_row_roots, d_col_roots, d_dah, d_status, d_workspace, s);
}

int dagpu_roots(dagpu_ctx* ctx, uint32_t k, const uint8_t* eds, uint8_t* row_roots,
                uint8_t* col_roots, uint8_t* dah) {
  if (!ctx || !eds || !row_roots || !col_roots || !dah) return DAGPU_ERR_ARG;
  std::lock_guard<std::mutex> g(ctx->mu);
  (void)hipSetDevice(ctx->device);
  int rc = check_k(ctx, k);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  HostResults res;
  HIP_TRY(ctx, ctx->eds.ensure(eds_bytes(k)));
  HIP_TRY(ctx, res.alloc(ctx, k, 1));
  HIP_TRY(ctx, ctx->ws.ensure(dagpu_workspace_size(k, 1)));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->eds.p, eds, eds_bytes(k), hipMemcpyHostToDevice, s));
  rc = enqueue_roots(ctx, k, 1, (const uint8_t*)ctx->eds.p, res.rr, res.cr, res.dah, res.st, ctx->ws.p, s);
  if (rc) return rc;
  HIP_TRY(ctx, res.download(ctx, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  int32_t st = 0;
  res.deliver(ctx, row_roots, col_roots, dah, &st);
  if (st & kStatusPushOrder)
    return set_err(ctx, DAGPU_ERR_PUSH_ORDER, "invalid push order: namespaces of original data square are not sorted");
  return DAGPU_OK;
}

int dagpu_encode(dagpu_ctx* ctx, uint32_t k, size_t nvec, size_t shard_size,
                 const uint8_t* data, uint8_t* parity) {
  if (!ctx || (nvec && (!data || !parity))) return DAGPU_ERR_ARG;
  if (shard_size == 0 || shard_size % 64)
    return set_err(ctx, DAGPU_ERR_SHARE_SIZE, "shard size must be a multiple of 64");
  std::lock_guard<std::mutex> g(ctx->mu);
  (void)hipSetDevice(ctx->device);
  int rc = check_codec_k(ctx, k);
  if (rc) return rc;
  if (nvec == 0) return DAGPU_OK;
  const size_t bytes = (size_t)k * shard_size * nvec;
  hipStream_t s = ctx->stream;
  HIP_TRY(ctx, ctx->ods.ensure(bytes));
  HIP_TRY(ctx, ctx->eds.ensure(bytes));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->ods.p, data, bytes, hipMemcpyHostToDevice, s));
  EncodeArgs ea{};
  ea.in = (const uint8_t*)ctx->ods.p;
  ea.out = (uint8_t*)ctx->eds.p;
  ea.copy = nullptr;
  ea.in_sq_stride = 0;
  ea.out_sq_stride = 0;
  ea.in_vec_stride = (long)k * (long)shard_size;
  ea.out_vec_stride = (long)k * (long)shard_size;
  ea.in_shard_stride = (long)shard_size;
  ea.out_shard_stride = (long)shard_size;
  ea.nsq = 1;
  ea.nvec = (long)nvec;
  ea.nchunk = (long)((shard_size + 511) / 512);
  ea.shard_bytes = (long)shard_size;
  HIP_TRY(ctx, launch_rs_encode((int)k, ea, s));
  HIP_TRY(ctx, hipMemcpyAsync(parity, ctx->eds.p, bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  return DAGPU_OK;
}

int dagpu_decode(dagpu_ctx* ctx, uint32_t k, size_t nvec, size_t shard_size, uint8_t* shards,
                 const uint8_t* present) {
  if (!ctx || (nvec && (!shards || !present))) return DAGPU_ERR_ARG;
  if (shard_size == 0 || shard_size % 64)
    return set_err(ctx, DAGPU_ERR_SHARE_SIZE, "shard size must be a multiple of 64");
  std::lock_guard<std::mutex> g(ctx->mu);
  (void)hipSetDevice(ctx->device);
  int rc = check_codec_k(ctx, k);
  if (rc) return rc;
  if (nvec == 0) return DAGPU_OK;
  const size_t n = 2 * (size_t)k;
  const size_t bytes = n * shard_size * nvec;
  hipStream_t s = ctx->stream;
  HIP_TRY(ctx, ctx->eds.ensure(bytes));
  HIP_TRY(ctx, ctx->ods.ensure(n * nvec));
  const size_t errb = (size_t)rs_err_bytes((int)k) * nvec;
  HIP_TRY(ctx, ctx->ws.ensure(errb + 3 * nvec * sizeof(int32_t) + 256));
  HIP_TRY(ctx, ctx->status.ensure(sizeof(int32_t)));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->eds.p, shards, bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->ods.p, present, n * nvec, hipMemcpyHostToDevice, s));
  HIP_TRY(ctx, hipMemsetAsync(ctx->status.p, 0, sizeof(int32_t), s));
  DecodeArgs da{};
  da.data = (uint8_t*)ctx->eds.p;
  da.sq_stride = 0;
  da.vec_stride = (long)(n * shard_size);
  da.shard_stride = (long)shard_size;
  da.present = (uint8_t*)ctx->ods.p;
  da.p_sq_stride = 0;
  da.p_vec_stride = (long)n;
  da.p_shard_stride = 1;
  da.err = (uint8_t*)ctx->ws.p;
  da.flags = (int32_t*)((uint8_t*)ctx->ws.p + errb);
  // locator sharing runs one workgroup over all vectors of a "square" (<= 2 kMaxK)
  da.err_key = nvec <= 2 * (size_t)kMaxK ? da.flags + nvec : nullptr;
  da.err_head = nvec <= 2 * (size_t)kMaxK ? da.flags + 2 * nvec : nullptr;
  da.too_few = (int32_t*)ctx->status.p;
  da.nsq = 1;
  da.nvec = (long)nvec;
  da.nchunk = (long)((shard_size + 511) / 512);
  da.shard_bytes = (long)shard_size;
  da.k = (int)k;
  {
    ProfScope p(ctx, 5, s);
    HIP_TRY(ctx, launch_rs_decode(da, s, false));
  }
  int32_t too_few = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&too_few, ctx->status.p, sizeof too_few, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipMemcpyAsync(shards, ctx->eds.p, bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  if (too_few) return set_err(ctx, DAGPU_ERR_TOO_FEW_SHARDS, "too few shards given");
  return DAGPU_OK;
}

int dagpu_profile_enable(dagpu_ctx* ctx, int on) {
  if (!ctx) return DAGPU_ERR_ARG;
  ctx->prof = (on & 1) != 0;
  ctx->stages_on = (on & 2) != 0;
  return DAGPU_OK;
}

int dagpu_profile_stages(dagpu_ctx* ctx, float* ms) {
  if (!ctx || !ms) return DAGPU_ERR_ARG;
  std::lock_guard<std::mutex> g(ctx->mu);
  for (int i = 0; i < dagpu_ctx::kStages; i++) ms[i] = -1.0f;
  if (!(ctx->stage_mask & 1u)) return DAGPU_OK;
  for (int i = 0; i < dagpu_ctx::kStages; i++) {
    if (!(ctx->stage_mask & (1u << i))) continue;
    HIP_TRY(ctx, hipEventSynchronize(ctx->stage_ev[i]));
    HIP_TRY(ctx, hipEventElapsedTime(&ms[i], ctx->stage_ev[0], ctx->stage_ev[i]));
  }
  return DAGPU_OK;
}

int dagpu_profile_read(dagpu_ctx* ctx, double* total_ms, uint64_t* launches, int reset) {
  if (!ctx) return DAGPU_ERR_ARG;
  std::lock_guard<std::mutex> g(ctx->prof_mu);
  for (auto& r : ctx->pending) {
    HIP_TRY(ctx, hipEventSynchronize(r.b));
    float ms = 0;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, r.a, r.b));
    ctx->prof_ms[r.id] += ms;
    ctx->prof_n[r.id] += 1;
    ctx->pool.push_back(r.a);
    ctx->pool.push_back(r.b);
  }
  ctx->pending.clear();
  for (int i = 0; i < DAGPU_PROFILE_KERNELS; i++) {
    if (total_ms) total_ms[i] = ctx->prof_ms[i];
    if (launches) launches[i] = ctx->prof_n[i];
    if (reset) { ctx->prof_ms[i] = 0; ctx->prof_n[i] = 0; }
  }
  return DAGPU_OK;
}

int dagpu_dah_hash(const uint8_t* row_roots, const uint8_t* col_roots, size_t w,
                   uint8_t* out32) {
  if (!out32 || (w && (!row_roots || !col_roots))) return DAGPU_ERR_ARG;
  std::vector<const uint8_t*> items;
  items.reserve(2 * w);
  for (size_t i = 0; i < w; i++) items.push_back(row_roots + i * kNodeSize);
  for (size_t i = 0; i < w; i++) items.push_back(col_roots + i * kNodeSize);
  host::rfc6962_root(items, kNodeSize, out32);
  return DAGPU_OK;
}

}  // extern "C"

#ifdef DAGPU_TEST_HOOKS
// Test build only (libdagpu_test.so, tests/test_gpu_rs_arms.py): launches per
// GF(2^8) kernel arm (kernels.hpp RsArm), counted by the dispatchers.
namespace dagpu {
namespace {
std::atomic<uint64_t> g_rs_arms[ARM_COUNT * kRsArmKs];
}
void rs_arm_launched(RsArm arm, int k) {
  int lg = 0;
  while ((1 << lg) < k && lg < kRsArmKs - 1) lg++;
  g_rs_arms[(int)arm * kRsArmKs + lg].fetch_add(1, std::memory_order_relaxed);
}
}  // namespace dagpu

// counts[arm * 8 + log2(k)] for the first n of the ARM_COUNT * 8 counters;
// reset != 0 zeroes all of them.  Returns the number of counters.
extern "C" int dagpu_test_rs_arms(uint64_t* counts, size_t n, int reset) {
  constexpr size_t total = (size_t)ARM_COUNT * kRsArmKs;
  for (size_t i = 0; i < total; i++) {
    const uint64_t c = reset ? g_rs_arms[i].exchange(0, std::memory_order_relaxed)
                             : g_rs_arms[i].load(std::memory_order_relaxed);
    if (counts && i < n) counts[i] = c;
  }
  return (int)total;
}
#endif
