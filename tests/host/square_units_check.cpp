// Stand-alone host check of csrc/square_units.hpp (no HIP, no library): reads
// cases { square, scan summary, records, expected unit table, unit bytes } from
// a file written by tests/test_square_units_check.py (every expectation there
// comes from the Python mirror), copies each square into a heap block of
// exactly its size, and runs
//   the host executor (squ_serial_square) into a table of exactly the expected
//   number of records,
//   the device algorithm as a host loop (squ_emulate_square), the per-lane
//   functions the kernels run, into another such table,
//   sqr_gather_window, the function each lane of the unit gather runs, for
//   every unit into a heap block of exactly len bytes.
// mode 0: both tables equal the expected one and the emulation says UNITS_OK;
// mode 1: the emulation must say UNITS_HOST, and the host executor returns the
// expected code; mode 2: UNITS_HOST, or UNITS_OK with the host executor's
// table.  Built with the address and undefined-behaviour sanitizers, a read one
// byte outside a square or a write one byte outside a table or a unit fails
// the run.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../celestia-app_amd/csrc/square_units.hpp"

using namespace dagpu;

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t cases = 0, shares = 0, units = 0, unit_bytes = 0, to_host = 0, refused = 0;
  if (!read_exact(f, &cases, 8)) return 2;
  for (uint64_t c = 0; c < cases; c++) {
    uint64_t hdr[5];  // k, records, expected units, mode, the host executor's return code
    int32_t scan[kSqrSummaryWords];
    if (!read_exact(f, hdr, sizeof hdr) || !read_exact(f, scan, sizeof scan)) return 2;
    const uint32_t k = (uint32_t)hdr[0], nrec = (uint32_t)hdr[1], mode = (uint32_t)hdr[3];
    const size_t bytes = (size_t)k * k * kSqShare, pitch = (size_t)k * kSqShare;
    // mode 0 knows the table's size; a broken square may yield any number of units
    const uint32_t cap = mode == 0 ? (uint32_t)hdr[2] : k * k * 256;
    uint8_t* sq = (uint8_t*)malloc(bytes);
    SqrRecord* rec = (SqrRecord*)malloc((nrec ? nrec : 1) * sizeof(SqrRecord));
    SquUnit* want = (SquUnit*)malloc((hdr[2] ? hdr[2] : 1) * sizeof(SquUnit));
    SquUnit* serial = (SquUnit*)malloc((cap ? cap : 1) * sizeof(SquUnit));
    SquUnit* lanes = (SquUnit*)malloc((cap ? cap : 1) * sizeof(SquUnit));
    if (!read_exact(f, sq, bytes) || !read_exact(f, rec, nrec * sizeof(SqrRecord)) ||
        !read_exact(f, want, hdr[2] * sizeof(SquUnit)))
      return 2;
    shares += (uint64_t)k * k;
    int32_t s_sum[kSqrSummaryWords], e_sum[kSqrSummaryWords];
    uint32_t bad = 0;
    const int rc = squ_serial_square(sq, k, pitch, rec, scan, nrec, cap, serial, s_sum, &bad);
    squ_emulate_square(sq, k, pitch, rec, scan, nrec, cap, lanes, e_sum);
    if (rc != (int)hdr[4]) {
      printf("case %llu: the host executor returned %d, expected %d\n", (unsigned long long)c, rc, (int)hdr[4]);
      return 1;
    }
    refused += rc != 0;
    const bool host = e_sum[0] == (int32_t)kUnitsHost;
    to_host += host;
    if (mode == 0) {
      if (s_sum[0] != (int32_t)kUnitsOk || (uint64_t)s_sum[2] != hdr[2] ||
          memcmp(serial, want, hdr[2] * sizeof(SquUnit)) != 0) {
        printf("case %llu: the host executor's table differs (%d units, expected %llu)\n", (unsigned long long)c,
               s_sum[2], (unsigned long long)hdr[2]);
        return 1;
      }
    } else if (mode == 1 && !host) {
      printf("case %llu: code %d where the square must go to the host\n", (unsigned long long)c, e_sum[0]);
      return 1;
    }
    if (!host && (rc != 0 || memcmp(e_sum, s_sum, sizeof s_sum) != 0 ||
                  memcmp(lanes, serial, (size_t)s_sum[2] * sizeof(SquUnit)) != 0)) {
      printf("case %llu: the lanes say code %d, %d units; the host executor %d, %d units\n", (unsigned long long)c,
             e_sum[0], e_sum[2], rc, s_sum[2]);
      return 1;
    }
    for (uint64_t u = 0; mode == 0 && u < hdr[2]; u++) {
      const SquUnit& w = want[u];
      const size_t len = (size_t)w.len;
      uint8_t* expect = (uint8_t*)malloc(len);
      uint8_t* out = (uint8_t*)malloc(len);
      if (!read_exact(f, expect, len)) return 2;
      memset(out, 0xA5, len);
      const uint32_t first = rec[w.seq].first;
      for (uint32_t j = squ::share_of((uint32_t)w.offset); j <= squ::share_of((uint32_t)(w.offset + len - 1)); j++)
        for (uint32_t lane = 0; lane < 64; lane++)
          sqr_gather_window(sq + (size_t)(first + j) * kSqShare, out, true, j, (uint32_t)w.offset, (uint32_t)len, lane);
      if (memcmp(out, expect, len) != 0) {
        printf("case %llu unit %llu: bytes differ\n", (unsigned long long)c, (unsigned long long)u);
        return 1;
      }
      units++;
      unit_bytes += len;
      free(expect);
      free(out);
    }
    free(sq);
    free(rec);
    free(want);
    free(serial);
    free(lanes);
  }
  fclose(f);
  printf("ok cases=%llu shares=%llu units=%llu bytes=%llu host=%llu refused=%llu\n", (unsigned long long)cases,
         (unsigned long long)shares, (unsigned long long)units, (unsigned long long)unit_bytes,
         (unsigned long long)to_host, (unsigned long long)refused);
  return 0;
}
