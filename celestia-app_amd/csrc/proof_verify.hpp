// proof_verify.hpp -- batched proof verification on the device
// (proof_verify.hip): nmt Proof.VerifyInclusion and crypto/merkle Proof.Verify
// for many proofs in three launches.  The host side (trees.cpp) validates every
// descriptor before anything here is launched; see include/dagpu.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dagpu {

constexpr int kPvDescNmt = 8;     // int64 per nmt descriptor (dagpu.h DAGPU_NMT_DESC_*)
constexpr int kPvDescNmtNs = 9;   // namespace proofs: the eight above + leaf_hash_index (DAGPU_NMT_NS_DESC_WORDS)
constexpr int kPvDescMerkle = 6;  // int64 per merkle descriptor
constexpr int kPvMaxHeight = 62;  // est = 2^H >= end, end <= 2^62
constexpr int kPvFoldLanes = 64;  // proofs per fold block (one wave)

// Records kept for a proof of nl leaves while its root is folded: the pending
// left siblings that overlap [start, end).  At most one contains `start`, at
// most one contains `end`, the others lie inside the range with distinct
// heights (2^h <= nl): bit_length(nl) + 2; one spare.
inline int pv_stack_depth(int64_t nl) {
  int b = 0;
  while (nl > 0) { b++; nl >>= 1; }
  return b + 3;
}

struct PvNmtArgs {
  long n;                  // proofs
  int namespace_rules;     // 0: VerifyInclusion; 1: VerifyNamespace (kPvDescNmtNs words, leaf_hashes)
  const int64_t* desc;     // n x kPvDescNmt (or kPvDescNmtNs), validated
  const int64_t* rec_off;  // n + 1: first leaf record of proof i (prefix sums)
  const int64_t* cs_off;   // n: first stack record of proof i; < 0 = range rejected
  const uint8_t* ns;       // namespace table, 29 B each
  const uint8_t* leaves;
  long leaf_len;
  int fast512;             // leaf_len == 512 and `leaves` 16-B aligned
  const uint8_t* nodes;    // packed 90-B nodes
  const uint8_t* roots;    // packed 90-B roots
  const uint8_t* leaf_hashes;  // packed 90-B leaf hashes of absence proofs (namespace_rules)
  uint8_t* recs;           // rec_off[n] leaf records (96 B)
  uint8_t* cstack;         // stack records (96 B)
  int32_t* status;
};

struct PvMerkleArgs {
  long n;
  const int64_t* desc;     // n x kPvDescMerkle, validated
  const uint8_t* leaves;
  long leaf_len;
  const uint8_t* leaf_hashes;  // n x 32 or null
  const uint8_t* aunts;        // 32 B each, 16-B aligned
  const uint8_t* roots;        // 32 B each, 16-B aligned
  int32_t* status;
};

hipError_t launch_pv_nmt_leaves(const PvNmtArgs& a, long n_records, hipStream_t s);
hipError_t launch_pv_nmt_fold(const PvNmtArgs& a, hipStream_t s);
hipError_t launch_pv_merkle(const PvMerkleArgs& a, hipStream_t s);

}  // namespace dagpu
