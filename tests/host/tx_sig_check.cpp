// Stand-alone host check of csrc/tx_sig.hpp and csrc/secp256k1.hpp
// (tests/test_tx_sig_host.py compiles and runs it, plain and with
// -fsanitize=address,undefined; no GPU, no HIP).  It runs the loops the host
// executors run (ts_run_raw_host behind dagpu_secp256k1_verify_host, ts_run_host
// behind dagpu_tx_sig_verify_host).  argv[1] names a file the test writes:
//   u32 count, then count x {pubkey[33], digest[32], sig[64], u32 expected word}
//   u32 n, one signed tx of n bytes; u32 chain id length, the chain id; u64 account number
// The raw items run in heap buffers of exactly their sizes and must give the
// expected words.  The tx runs
//   * as every prefix, lengths 0 .. n,
//   * with each byte replaced by 0x00, 0x7F, 0x80 and 0xFF in turn,
// each input in a heap buffer of exactly its length, so a read at or past n is
// an AddressSanitizer report; a defined kind must come back, 0 for the tx
// itself.  Prints "OK key=value ..." for the Python side.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "tx_sig.hpp"

using namespace dagpu;

static bool defined_kind(uint32_t w) {
  const uint32_t k = w & 0xFF;
  return k <= kSigNoPubkey || (k >= kSigBadPubkey && k <= kSigMismatch);
}

// the word of a copy of b[0, n) that owns exactly n bytes, as a block of one tx
static uint32_t check_exact(const uint8_t* b, size_t n, const std::vector<uint8_t>& chain, uint64_t acct,
                            uint32_t* block_words, uint8_t* signer) {
  uint8_t* own = n ? new uint8_t[n] : nullptr;
  if (n) memcpy(own, b, n);
  const TsCarve c = ts_carve(1, 1);
  std::vector<uint64_t> ws(c.total / 8 + 1);
  uint8_t* w = (uint8_t*)ws.data();
  memset(w, 0xFF, 8);
  const SpBlockIn blk = {0, 0, (uint32_t)n, 0, 1, 0};
  const SpTxIn tx = {0, (uint32_t)n, 0, 0};
  memcpy(w + c.blk, &blk, sizeof blk);
  memcpy(w + c.tx, &tx, sizeof tx);
  if (!chain.empty()) memcpy(w + c.chain, chain.data(), chain.size());
  uint32_t status = 0xEEEEEEEEu;
  const TsArgs a = ts_args(w, own, 1, 1, (uint32_t)chain.size(), &acct, nullptr, true, signer, &status, block_words);
  ts_run_host(a);
  delete[] own;
  return status;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> in;
  for (int c; (c = fgetc(f)) != EOF;) in.push_back((uint8_t)c);
  fclose(f);
  size_t at = 0;
  auto u32 = [&]() {
    uint32_t v;
    memcpy(&v, in.data() + at, 4);
    at += 4;
    return v;
  };

  // ---- the raw call ----
  const uint32_t count = u32();
  uint8_t* pk = new uint8_t[33 * (size_t)count];
  uint8_t* dg = new uint8_t[32 * (size_t)count];
  uint8_t* sg = new uint8_t[64 * (size_t)count];
  std::vector<uint32_t> want(count), got(count, 0xEEEEEEEEu);
  for (uint32_t i = 0; i < count; i++) {
    memcpy(pk + 33 * i, in.data() + at, 33);
    memcpy(dg + 32 * i, in.data() + at + 33, 32);
    memcpy(sg + 64 * i, in.data() + at + 65, 64);
    at += 129;
    want[i] = u32();
  }
  ts_run_raw_host(ts_raw_args(count, dg, sg, pk, got.data()));
  delete[] pk;
  delete[] dg;
  delete[] sg;
  for (uint32_t i = 0; i < count; i++)
    if (got[i] != want[i]) {
      printf("FAIL raw item %u: word %u, expected %u\n", i, got[i], want[i]);
      return 1;
    }

  // ---- one signed tx ----
  const uint32_t n = u32();
  const std::vector<uint8_t> tx(in.begin() + at, in.begin() + at + n);
  at += n;
  const uint32_t chain_len = u32();
  const std::vector<uint8_t> chain(in.begin() + at, in.begin() + at + chain_len);
  at += chain_len;
  uint64_t acct;
  memcpy(&acct, in.data() + at, 8);

  uint32_t block_words[4];
  uint8_t signer[kTsSigner];
  const uint32_t valid = check_exact(tx.data(), n, chain, acct, block_words, signer);
  std::string prefix_words;
  size_t prefixes = 0, substitutions = 0, reached_curve = 0;
  for (size_t len = 0; len <= n; len++, prefixes++) {
    const uint32_t w = check_exact(tx.data(), len, chain, acct, block_words, signer);
    if (!defined_kind(w)) {
      printf("FAIL prefix %zu: word %u\n", len, w);
      return 1;
    }
    prefix_words += (len ? "," : "") + std::to_string(w);
  }
  const uint8_t subs[4] = {0x00, 0x7F, 0x80, 0xFF};
  std::vector<uint8_t> m = tx;
  for (size_t i = 0; i < n; i++) {
    for (uint8_t s : subs) {
      if (s == tx[i]) continue;
      m[i] = s;
      const uint32_t w = check_exact(m.data(), n, chain, acct, block_words, signer);
      if (!defined_kind(w)) {
        printf("FAIL byte %zu = %u: word %u\n", i, s, w);
        return 1;
      }
      reached_curve += (w & 0xFF) >= kSigOutOfRange || w == kSigOk;
      substitutions++;
    }
    m[i] = tx[i];
  }
  printf("OK raw=%u valid=%u prefixes=%zu substitutions=%zu reached_curve=%zu prefix_words=%s\n", count, valid,
         prefixes, substitutions, reached_curve, prefix_words.c_str());
  return 0;
}
