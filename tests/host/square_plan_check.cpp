// Stand-alone host check of csrc/square_plan.hpp: the device planner's
// algorithm as host loops (sp_emulate: the per-lane functions the kernels run,
// 256 lanes per phase), compiled into this program so that the address and
// undefined-behaviour sanitizers see every read of the txs and every write of
// the tables.  Reads cases { max_square_size, tx lengths, txs, the expected
// status and plan } from a file written by tests/test_square_plan_device_host.py
// (every expectation there comes from the host planner, dagpu_square_plan),
// copies each block's txs into a heap block of exactly their size, the arena
// into one of exactly the documented bound, and checks
//   the status word's kind (and index where the case gives one),
//   the plan byte for byte,
//   dagpu_square_plan_check (from libdagpu) on every emitted plan.
// First it compares the integer blob_min_square_size / subtree_width_u of the
// header with the double forms they replaced, for every share count 0 ..
// 128^2 + 1 and thresholds 1, 64, 128.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "../../celestia-app_amd/csrc/square_plan.hpp"
#include "../../include/dagpu.h"

using namespace dagpu;

// libdagpu brings the HIP runtime with it, whose start-up allocations are not this program's
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static uint64_t double_min_square_size(uint64_t share_count) {
  uint64_t v = (uint64_t)ceil(sqrt((double)share_count)), r = 1;
  while (r < v) r <<= 1;
  return r;
}
static uint64_t double_subtree_width(uint64_t share_count, uint64_t threshold) {
  uint64_t s = share_count / threshold + (share_count % threshold ? 1 : 0), r = 1;
  while (r < s) r <<= 1;
  const uint64_t m = double_min_square_size(share_count);
  return r < m ? r : m;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  uint64_t widths = 0;
  for (uint64_t n = 0; n <= 128 * 128 + 1; n++) {
    if (blob_min_square_size(n) != double_min_square_size(n)) {
      printf("blob_min_square_size(%llu) differs\n", (unsigned long long)n);
      return 1;
    }
    for (uint64_t t : {1, 64, 128}) {
      if (subtree_width_u(n, t) != double_subtree_width(n, t)) {
        printf("subtree_width_u(%llu, %llu) differs\n", (unsigned long long)n, (unsigned long long)t);
        return 1;
      }
      widths++;
    }
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t cases = 0, txs = 0, bytes = 0, plans = 0, rejected = 0;
  if (!read_exact(f, &cases, 8)) return 2;
  SpShared* shared = (SpShared*)malloc(sizeof(SpShared));
  for (uint64_t c = 0; c < cases; c++) {
    uint64_t hdr[5];  // max_square_size, ntx, expected kind, expected index or ~0, expected plan bytes
    if (!read_exact(f, hdr, sizeof hdr)) return 2;
    const uint32_t m = (uint32_t)hdr[0], ntx = (uint32_t)hdr[1];
    uint64_t* lens = (uint64_t*)malloc((ntx ? ntx : 1) * 8);
    if (!read_exact(f, lens, ntx * 8)) return 2;
    uint64_t total = 0;
    for (uint32_t i = 0; i < ntx; i++) total += lens[i];
    uint8_t* src = (uint8_t*)malloc(total);
    uint8_t* want = (uint8_t*)malloc(hdr[4]);
    if (!read_exact(f, src, total) || !read_exact(f, want, hdr[4])) return 2;
    const SpCarve cv = sp_carve(1, ntx, m);
    uint8_t* ws = (uint8_t*)calloc(cv.total, 1);
    const uint64_t cap = sp_up16(sp_plan_bound(ntx, m));
    uint8_t* arena = (uint8_t*)malloc(cap);
    memset(arena, 0xA5, cap);
    SpBlockIn* blk = (SpBlockIn*)(ws + cv.blk);
    SpTxIn* tx = (SpTxIn*)(ws + cv.tx);
    *blk = {0, 0, (uint32_t)total, 0, ntx, 0};
    uint32_t off = 0;
    for (uint32_t i = 0; i < ntx; i++) {
      tx[i] = {off, (uint32_t)lens[i], 0, 0};
      off += (uint32_t)lens[i];
    }
    SpRecord rec;
    uint32_t status = 0xFFFFFFFFu;
    SpArgs a;
    a.src = src;
    a.blk = blk;
    a.tx = tx;
    a.cls = (SpTxCls*)(ws + cv.cls);
    a.pos = (SpTxPos*)(ws + cv.pos);
    a.sorted = (uint16_t*)(ws + cv.sorted);
    a.blobs = (SpBlobRec*)(ws + cv.blobs);
    a.arena = arena;
    a.arena_cap = cap;
    a.cursor = (unsigned long long*)ws;
    a.clocks = (unsigned long long*)(ws + cv.clocks);
    a.rec = &rec;
    a.status = &status;
    a.n = 1;
    a.max_square_size = m;
    a.threshold = 64;
    sp_emulate(a, ntx, *shared);
    const uint32_t kind = status & 0xFF, index = status >> 8;
    if (kind != hdr[2] || (hdr[3] != ~0ull && index != hdr[3])) {
      printf("case %llu: status %u index %u, expected %llu index %lld\n", (unsigned long long)c, kind, index,
             (unsigned long long)hdr[2], (long long)hdr[3]);
      return 1;
    }
    if (kind == 0) {
      if (rec.plan_bytes != hdr[4] || rec.plan_off != 0 || memcmp(arena, want, hdr[4]) != 0) {
        printf("case %llu: the plan differs (%u bytes, expected %llu)\n", (unsigned long long)c, rec.plan_bytes,
               (unsigned long long)hdr[4]);
        return 1;
      }
      if (dagpu_square_plan_check(arena, rec.plan_bytes, total) != DAGPU_OK) {
        printf("case %llu: dagpu_square_plan_check: %s\n", (unsigned long long)c, dagpu_last_error(NULL));
        return 1;
      }
      plans++;
    } else {
      rejected++;
    }
    for (uint64_t i = kind == 0 ? rec.plan_bytes : 0; i < cap; i++)
      if (arena[i] != 0xA5) {
        printf("case %llu: arena byte %llu written outside the plan\n", (unsigned long long)c, (unsigned long long)i);
        return 1;
      }
    txs += ntx;
    bytes += total;
    free(lens);
    free(src);
    free(want);
    free(ws);
    free(arena);
  }
  free(shared);
  fclose(f);
  printf("ok cases=%llu txs=%llu bytes=%llu plans=%llu rejected=%llu widths=%llu\n", (unsigned long long)cases,
         (unsigned long long)txs, (unsigned long long)bytes, (unsigned long long)plans, (unsigned long long)rejected,
         (unsigned long long)widths);
  return 0;
}
