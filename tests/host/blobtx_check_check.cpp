// Stand-alone host check of csrc/blobtx_check.hpp (tests/test_blobtx_validate_host.py
// compiles and runs it, plain and with -fsanitize=address,undefined; no GPU, no
// HIP).  argv[1] names a file holding one valid BlobTx.  bt_check_tx is fed
//   * every prefix of the tx, lengths 0 .. n,
//   * the tx with each byte outside its blobs' data replaced by 0x00, 0x7F,
//     0x80 and 0xFF in turn,
// each input in a heap buffer of exactly its length, so a read at or past n is
// an AddressSanitizer report.  The only assertion is that a defined kind comes
// back.  Prints "OK key=value ..." for the Python side.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "blobtx_check.hpp"

using namespace dagpu;

// the word of a copy of b[0, n) that owns exactly n bytes
static uint32_t check_exact(const uint8_t* b, size_t n) {
  uint8_t* own = n ? new uint8_t[n] : nullptr;
  if (n) memcpy(own, b, n);
  BtTxInfo info;
  const uint32_t w = bt_check_tx(own, (uint32_t)n, &info);
  delete[] own;
  return w;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> tx;
  for (int c; (c = fgetc(f)) != EOF;) tx.push_back((uint8_t)c);
  fclose(f);
  const size_t n = tx.size();

  const uint32_t valid = check_exact(tx.data(), n);
  std::vector<bool> is_data(n, false);
  {
    SpBlobFields b;
    uint32_t at = 0;
    while (bt_next_blob(tx.data(), (uint32_t)n, at, b) > 0)
      for (uint32_t i = 0; i < b.data_len; i++) is_data[b.data_off + i] = true;
  }

  std::string prefix_kinds;
  size_t prefixes = 0, substitutions = 0;
  for (size_t len = 0; len <= n; len++, prefixes++) {
    const uint32_t w = check_exact(tx.data(), len);
    if ((w & 0xFF) >= kBtKinds) {
      printf("FAIL prefix %zu: word %u\n", len, w);
      return 1;
    }
    prefix_kinds += (len ? "," : "") + std::to_string(w & 0xFF);
  }
  const uint8_t subs[4] = {0x00, 0x7F, 0x80, 0xFF};
  std::vector<uint8_t> m = tx;
  for (size_t i = 0; i < n; i++) {
    if (is_data[i]) continue;
    for (uint8_t s : subs) {
      m[i] = s;
      const uint32_t w = check_exact(m.data(), n);
      if ((w & 0xFF) >= kBtKinds) {
        printf("FAIL byte %zu = %u: word %u\n", i, s, w);
        return 1;
      }
      substitutions++;
    }
    m[i] = tx[i];
  }
  printf("OK valid=%u prefixes=%zu substitutions=%zu prefix_kinds=%s\n", valid, prefixes, substitutions,
         prefix_kinds.c_str());
  return 0;
}
