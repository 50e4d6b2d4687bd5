// Stand-alone host check of csrc/square_write.hpp (no HIP, no library): reads
// cases { plan, packed txs, expected ODS } from a file written by
// tests/test_square_write_host.py, copies plan and txs into heap blocks of
// exactly their sizes, computes every share with sq_share_desc + sq_share_word
// (the functions the kernel runs) and compares with the expected bytes.  Built
// with the address and undefined-behaviour sanitizers, a read one byte outside
// a plan or its txs fails the run.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../celestia-app_amd/csrc/square_write.hpp"

using namespace dagpu;

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t cases = 0, shares = 0, seam_words = 0;
  if (!read_exact(f, &cases, 8)) return 2;
  for (uint64_t c = 0; c < cases; c++) {
    uint64_t hdr[3];  // plan bytes, txs bytes, k
    if (!read_exact(f, hdr, sizeof hdr)) return 2;
    const uint64_t k = hdr[2];
    uint8_t* plan = (uint8_t*)malloc(hdr[0] ? hdr[0] : 1);
    uint8_t* src = (uint8_t*)malloc(hdr[1] ? hdr[1] : 1);
    std::vector<uint8_t> want(k * k * kSqShare), got(kSqShare);
    if (!read_exact(f, plan, hdr[0]) || !read_exact(f, src, hdr[1]) || !read_exact(f, want.data(), want.size()))
      return 2;
    const SqHdr* h = (const SqHdr*)plan;
    if (h->k != k || h->plan_bytes != hdr[0]) return 3;
    for (uint32_t s = 0; s < k * k; s++) {
      const SqShareDesc d = sq_share_desc(plan, s);
      for (uint32_t i = 0; i < kSqShare / 8; i++) {
        const uint64_t w = sq_share_word(d, plan + h->lit_off, src, i);
        memcpy(got.data() + 8 * i, &w, 8);
      }
      if (memcmp(got.data(), want.data() + (size_t)s * kSqShare, kSqShare) != 0) {
        printf("case %llu share %u differs\n", (unsigned long long)c, s);
        return 1;
      }
      if (d.mode == 1) seam_words += d.hi - d.lo;  // segment seams inside this share
      shares++;
    }
    free(plan);
    free(src);
  }
  fclose(f);
  printf("ok cases=%llu shares=%llu seams=%llu\n", (unsigned long long)cases, (unsigned long long)shares,
         (unsigned long long)seam_words);
  return 0;
}
