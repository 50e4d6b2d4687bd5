// Stand-alone host check of csrc/square_read.hpp (no HIP, no library): reads
// cases { square, expected summary, records, payloads, units } from a file
// written by tests/test_square_read_check.py (every expectation there comes
// from the Python mirror), copies each square into a heap block of exactly its
// size, runs the host executor (sqr_scan_square), then gathers every
// non-padding sequence with sqr_gather_lane (the function each lane of the
// gather kernel runs) into a heap block of exactly payload_len bytes and walks
// the compact ones with sqr_compact_units.  Built with the address and
// undefined-behaviour sanitizers, a read one byte outside a square or a write
// one byte outside a payload fails the run.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../celestia-app_amd/csrc/square_read.hpp"

using namespace dagpu;

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t cases = 0, shares = 0, records = 0, payload_bytes = 0, units = 0, edge_words = 0;
  if (!read_exact(f, &cases, 8)) return 2;
  for (uint64_t c = 0; c < cases; c++) {
    uint64_t hdr[4];  // k, seq_cap, expected records, 1 = compare records and content
    int32_t want_sum[kSqrSummaryWords], got_sum[kSqrSummaryWords];
    if (!read_exact(f, hdr, sizeof hdr) || !read_exact(f, want_sum, sizeof want_sum)) return 2;
    const uint32_t k = (uint32_t)hdr[0], cap = (uint32_t)hdr[1];
    const size_t nrec = hdr[2], bytes = (size_t)k * k * kSqShare;
    uint8_t* sq = (uint8_t*)malloc(bytes);
    SqrRecord* got = (SqrRecord*)malloc((cap ? cap : 1) * sizeof(SqrRecord));
    std::vector<SqrRecord> want(nrec);
    if (!read_exact(f, sq, bytes) || !read_exact(f, want.data(), nrec * sizeof(SqrRecord))) return 2;
    sqr_scan_square(sq, k, (size_t)k * kSqShare, cap, got, got_sum);
    shares += (uint64_t)k * k;
    const size_t cmp = hdr[3] ? sizeof got_sum : 3 * sizeof(int32_t);
    if (memcmp(got_sum, want_sum, cmp) != 0) {
      printf("case %llu: summary {%d %d %d %d ..} expected {%d %d %d %d ..}\n", (unsigned long long)c, got_sum[0],
             got_sum[1], got_sum[2], got_sum[3], want_sum[0], want_sum[1], want_sum[2], want_sum[3]);
      return 1;
    }
    if (hdr[3]) {
      if (memcmp(got, want.data(), nrec * sizeof(SqrRecord)) != 0) {
        printf("case %llu: records differ\n", (unsigned long long)c);
        return 1;
      }
      for (size_t r = 0; r < nrec; r++) {
        const SqrRecord& q = want[r];
        records++;
        if (q.flags & kSeqPadding) continue;
        const bool compact = !(q.flags & kSeqSparse);
        uint8_t* expect = (uint8_t*)malloc(q.payload ? q.payload : 1);
        uint8_t* out = (uint8_t*)malloc(q.payload ? q.payload : 1);
        if (!read_exact(f, expect, q.payload)) return 2;
        memset(out, 0xA5, q.payload);
        for (uint32_t j = 0; j < q.count; j++) {
          for (uint32_t lane = 0; lane < 64; lane++)
            sqr_gather_lane(sq + (size_t)(q.first + j) * kSqShare, out, compact, j, q.payload, lane);
          edge_words += (sqr_stream_pos(compact, j) & 7) != 0;
        }
        if (memcmp(out, expect, q.payload) != 0) {
          printf("case %llu record %zu: payload differs\n", (unsigned long long)c, r);
          return 1;
        }
        payload_bytes += q.payload;
        if (compact) {
          uint64_t n_want = 0;
          if (!read_exact(f, &n_want, 8)) return 2;
          std::vector<uint64_t> w(2 * n_want), off(n_want + 1), len(n_want + 1);
          if (!read_exact(f, w.data(), 16 * n_want)) return 2;
          size_t n = 0;
          if (sqr_compact_units(out, q.payload, q.reserved, off.data(), len.data(), n_want + 1, &n) != 0 ||
              n != n_want) {
            printf("case %llu record %zu: %zu units, expected %llu\n", (unsigned long long)c, r, n,
                   (unsigned long long)n_want);
            return 1;
          }
          for (size_t u = 0; u < n; u++)
            if (off[u] != w[2 * u] || len[u] != w[2 * u + 1]) {
              printf("case %llu record %zu unit %zu differs\n", (unsigned long long)c, r, u);
              return 1;
            }
          units += n;
        }
        free(expect);
        free(out);
      }
    }
    free(sq);
    free(got);
  }
  fclose(f);
  printf("ok cases=%llu shares=%llu records=%llu payload=%llu units=%llu edges=%llu\n", (unsigned long long)cases,
         (unsigned long long)shares, (unsigned long long)records, (unsigned long long)payload_bytes,
         (unsigned long long)units, (unsigned long long)edge_words);
  return 0;
}
