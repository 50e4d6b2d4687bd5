// blobtx_check.hpp -- the stateless rules ProcessProposal applies to every tx of
// a block before it builds the square (app/process_proposal.go:60-77 and :120),
// in one copy for the host (blobtx_host.cpp: dagpu_blob_tx_check,
// dagpu_blob_tx_validate_host) and the device (blobtx_check.hip,
// dagpu_blob_tx_validate_device).  Plain arithmetic only (no HIP include);
// every function is marked for both sides when hipcc compiles it.
//
// bt_check_tx takes the n bytes of one tx and returns a status word
// kind | index << 8 (the planner's convention, square_plan.hpp); it never reads
// a byte at or past n.
//
// A BlobTx (sp_unmarshal_blob_tx says so) goes through ValidateBlobTx
// (x/blob/types/blob_tx.go:36-103) up to, and without, the comparison of the
// commitments themselves (blob_tx.go:92-100: dagpu_blob_commitments_device
// makes it against the table bt_tie_row fills).  The first failure wins:
//   kBtDecode          the inner tx does not decode (blob_tx.go:37-40): a
//                      malformed buffer, or a wrong wire type for Body (Tx 1),
//                      Messages (TxBody 1), TypeUrl (Any 1) or Value (Any 2).
//                      The SDK's TxDecoder is not in the reference: the walker
//                      this project already has (celestia_da/blobtx.py
//                      sdk_tx_messages) is the rule, and the SDK's stricter
//                      rejections (unknown non-critical fields, unregistered
//                      type urls, signer counts) are not restated.
//   kBtMultipleMsgs    message count != 1, 0 included (blob_tx.go:44-47);
//                      index = the count, capped at 2^24 - 1
//   kBtNoPfb           the message's type_url is not /celestia.blob.v1.MsgPayForBlobs (:49-52)
//   kBtPfbDecode       the message value is malformed, or a wrong wire type on
//                      fields 1, 2, 3, 4 or 8 (the unpack behind :49)
//   MsgPayForBlobs.ValidateBasic (x/blob/types/payforblob.go:95-148), line for line:
//   kBtNoNamespaces, kBtNoShareVersions, kBtNoBlobSizes, kBtNoShareCommitments  (:96-110)
//   kBtMismatchedCounts                                                        (:112-117)
//   kBtInvalidNamespace        namespace.From fails (:120-123), index = the namespace
//   kBtReservedNamespace       IsReserved (payforblob.go:184, namespace.go:108-118)
//   kBtInvalidNamespaceVersion not in SupportedBlobNamespaceVersions (:188):
//                      reachable, a version-255 namespace below the secondary
//                      reserved range passes From and IsReserved
//   kBtUnsupportedShareVersion  index = the share version (:130-134)
//   kBtBadSigner       sdk.AccAddressFromBech32 with the prefix "celestia"
//                      (:136-139).  The SDK is not vendored in the reference:
//                      the rule below (bt_signer_ok) is recalled from BIP-173
//                      and the SDK's published source, parity unpinned; the
//                      only anchors are the addresses the reference's own
//                      files contain (tests/test_blobtx_validate_host.py).
//   kBtBadCommitmentLength  index = the commitment (:141-145)
//   ValidateBlobs over the BlobTx's blobs, ascending (payforblob.go:211-239);
//   index = the blob:
//   kBtBlobNsVersionTooLarge (:217), kBtBlobInvalidNamespace (namespace.New, :220),
//   kBtBlobReservedNamespace, kBtBlobInvalidNamespaceVersion (:224),
//   kBtZeroBlobSize (:229), kBtBlobUnsupportedShareVersion (:233, on the low 8
//   bits of the field as the reference's uint8 conversion takes them)
//   kBtSizeMismatch    blob_tx.go:69: the blob count != the number of declared
//                      sizes (index = the smaller count), or the first blob
//                      whose len(data) != blob_sizes[i]
//   kBtNamespaceMismatch  blob_tx.go:73-89: the lowest i whose blob namespace
//                      differs from namespaces[i]
// ErrNoBlobs (payforblob.go:212) has no kind: a BlobTx without blobs is not a
// BlobTx (blob.UnmarshalBlobTx), and the errors of From / New at blob_tx.go:74-84
// cannot occur behind ValidateBasic and ValidateBlobs.  Every kind above is
// reachable; tests/test_blobtx_validate_host.py holds one tx for each.
//
// A tx that is not a BlobTx (process_proposal.go:60-77) is walked the same
// way: if any step of the walk fails the word is 0 (an undecodable tx is not a
// validity fault), if some message's type_url is the PFB url the word is
// kBtNonBlobTxHasPfb with index = the first such message, else 0.
#pragma once
#include <stdint.h>

#include "square_plan.hpp"

// The rules a lane runs once per tx are inlined into the kernel: a call would
// spill the caller's registers to scratch.
#define DAGPU_BT_INLINE inline __attribute__((always_inline))

namespace dagpu {

enum : uint32_t {
  kBtOk = 0,
  kBtDecode = 1,
  kBtMultipleMsgs = 2,
  kBtNoPfb = 3,
  kBtPfbDecode = 4,
  kBtNoNamespaces = 5,
  kBtNoShareVersions = 6,
  kBtNoBlobSizes = 7,
  kBtNoShareCommitments = 8,
  kBtMismatchedCounts = 9,
  kBtInvalidNamespace = 10,
  kBtReservedNamespace = 11,
  kBtInvalidNamespaceVersion = 12,
  kBtUnsupportedShareVersion = 13,
  kBtBadSigner = 14,
  kBtBadCommitmentLength = 15,
  kBtBlobNsVersionTooLarge = 16,
  kBtBlobInvalidNamespace = 17,
  kBtBlobReservedNamespace = 18,
  kBtBlobInvalidNamespaceVersion = 19,
  kBtZeroBlobSize = 20,
  kBtBlobUnsupportedShareVersion = 21,
  kBtSizeMismatch = 22,
  kBtNamespaceMismatch = 23,
  kBtNonBlobTxHasPfb = 24,
  kBtKinds = 25,
};
constexpr uint32_t kBtNone = 0xFFFFFFFFu;
constexpr uint32_t kBtNsSize = 29;
constexpr uint32_t kBtCommitment = 32;
constexpr uint32_t kBtUrlLen = 32;

DAGPU_SQ_HD inline uint32_t bt_word(uint32_t kind, uint64_t index) {
  return kind | (uint32_t)(index > 0xFFFFFFu ? 0xFFFFFFu : index) << 8;
}

// ---- the messages of a cosmos Tx ------------------------------------------------
// Tx {body 1} -> TxBody {messages 1} -> Any {type_url 1, value 2}.  Messages of
// every body field accumulate; inside an Any the last of each field wins.
struct BtMsgs {
  uint32_t count;
  uint32_t url_off, url_len, val_off, val_len;  // of message 0, from the start of the buffer
  uint32_t first_pfb;                           // the first message with the PFB url, or kBtNone
};
DAGPU_SQ_HD inline bool bt_is_pfb_url(const uint8_t* p, uint32_t len) {
  const char* url = "/celestia.blob.v1.MsgPayForBlobs";
  if (len != kBtUrlLen) return false;
  for (uint32_t i = 0; i < kBtUrlLen; i++)
    if (p[i] != (uint8_t)url[i]) return false;
  return true;
}
// false: the buffer does not decode
DAGPU_SQ_HD inline bool bt_walk_msgs(const uint8_t* b, uint32_t n, BtMsgs& m) {
  m.count = m.url_off = m.url_len = m.val_off = m.val_len = 0;
  m.first_pfb = kBtNone;
  uint32_t i = 0;
  SpField f, g, h;
  for (;;) {
    const int st = sp_next_field(b, n, i, f);
    if (st < 0) return false;
    if (st == 0) return true;
    if (f.num != 1) continue;
    if (f.wt != 2) return false;
    uint32_t j = 0;
    for (;;) {
      const int s2 = sp_next_field(b + f.off, f.len, j, g);
      if (s2 < 0) return false;
      if (s2 == 0) break;
      if (g.num != 1) continue;
      if (g.wt != 2) return false;
      const uint32_t any = f.off + g.off;
      uint32_t q = 0, url_off = 0, url_len = 0, val_off = 0, val_len = 0;
      for (;;) {
        const int s3 = sp_next_field(b + any, g.len, q, h);
        if (s3 < 0) return false;
        if (s3 == 0) break;
        if (h.num == 1) {
          if (h.wt != 2) return false;
          url_off = any + h.off;
          url_len = h.len;
        } else if (h.num == 2) {
          if (h.wt != 2) return false;
          val_off = any + h.off;
          val_len = h.len;
        }
      }
      if (m.count == 0) {
        m.url_off = url_off;
        m.url_len = url_len;
        m.val_off = val_off;
        m.val_len = val_len;
      }
      if (m.first_pfb == kBtNone && bt_is_pfb_url(b + url_off, url_len)) m.first_pfb = m.count;
      m.count++;
    }
  }
}

// ---- namespaces -------------------------------------------------------------------
// namespace.From / New and ValidateBlobNamespace over the 29 bytes byte(0..28):
// 0 valid, 1 From / New fails, 2 reserved, 3 the version is no blob version.
// Primary reserved: <= 0x00 | 27 zeros | 0xFF; secondary: >= 0xFF | 27 x 0xFF | 0x00
// (pkg/namespace/consts.go:38-65).
template <class B>
DAGPU_SQ_HD DAGPU_BT_INLINE uint32_t bt_namespace_rule(B&& byte) {
  if (namespace_fault_of(byte)) return 1;
  const uint8_t v = byte(0);
  bool same = true;  // bytes 1..27 all equal the version byte (0x00 or 0xFF)
  for (uint32_t i = 1; i <= 27; i++) same = same && byte(i) == v;
  if (same) return 2;
  return v == 0 ? 0 : 3;
}

// ---- sdk.AccAddressFromBech32 ---------------------------------------------------
// -1: not in the bech32 alphabet
DAGPU_SQ_HD DAGPU_BT_INLINE int bt_bech32_value(uint8_t c) {
  switch (c) {
    case 'q': return 0;
    case 'p': return 1;
    case 'z': return 2;
    case 'r': return 3;
    case 'y': return 4;
    case '9': return 5;
    case 'x': return 6;
    case '8': return 7;
    case 'g': return 8;
    case 'f': return 9;
    case '2': return 10;
    case 't': return 11;
    case 'v': return 12;
    case 'd': return 13;
    case 'w': return 14;
    case '0': return 15;
    case 's': return 16;
    case '3': return 17;
    case 'j': return 18;
    case 'n': return 19;
    case '5': return 20;
    case '4': return 21;
    case 'k': return 22;
    case 'h': return 23;
    case 'c': return 24;
    case 'e': return 25;
    case '6': return 26;
    case 'm': return 27;
    case 'u': return 28;
    case 'a': return 29;
    case '7': return 30;
    case 'l': return 31;
    default: return -1;
  }
}
DAGPU_SQ_HD inline uint32_t bt_polymod_step(uint32_t chk, uint32_t v) {
  const uint32_t top = chk >> 25;
  chk = (chk & 0x1FFFFFFu) << 5 ^ v;
  if (top & 1) chk ^= 0x3B6A57B2u;
  if (top & 2) chk ^= 0x26508E6Du;
  if (top & 4) chk ^= 0x1EA119FAu;
  if (top & 8) chk ^= 0x3D4233DDu;
  if (top & 16) chk ^= 0x2A1462B3u;
  return chk;
}
DAGPU_SQ_HD inline uint8_t bt_lower(uint8_t c) { return c >= 'A' && c <= 'Z' ? (uint8_t)(c + 32) : c; }
// The signer s[0, n): non-empty after trimming spaces; BIP-173 bech32 (every
// char in 33..126, not mixed case, a '1' separator with >= 1 char before and
// >= 6 after it, data chars in the alphabet, polymod over the expanded HRP and
// the data = 1); HRP "celestia"; the 5 -> 8 bit regrouping without padding
// (leftover bits < 5 and all zero); 1 to 255 bytes.
DAGPU_SQ_HD DAGPU_BT_INLINE bool bt_signer_ok(const uint8_t* s, uint32_t n) {
  uint32_t lead = 0, end = n;
  while (lead < end && s[lead] == ' ') lead++;
  while (end > lead && s[end - 1] == ' ') end--;
  if (lead == end) return false;
  bool lower = false, upper = false;
  uint32_t sep = kBtNone;
  for (uint32_t i = 0; i < n; i++) {
    const uint8_t c = s[i];
    if (c < 33 || c > 126) return false;
    lower = lower || (c >= 'a' && c <= 'z');
    upper = upper || (c >= 'A' && c <= 'Z');
    if (c == '1') sep = i;
  }
  if (lower && upper) return false;
  if (sep == kBtNone || sep < 1 || n - sep - 1 < 6) return false;
  const char* hrp = "celestia";
  if (sep != 8) return false;
  uint32_t chk = 1;
  for (uint32_t i = 0; i < 8; i++) {
    if (bt_lower(s[i]) != (uint8_t)hrp[i]) return false;
    chk = bt_polymod_step(chk, (uint32_t)hrp[i] >> 5);
  }
  chk = bt_polymod_step(chk, 0);
  for (uint32_t i = 0; i < 8; i++) chk = bt_polymod_step(chk, (uint32_t)hrp[i] & 31);
  uint32_t acc = 0, bits = 0, bytes = 0;
  for (uint32_t i = sep + 1; i < n; i++) {
    const int v = bt_bech32_value(bt_lower(s[i]));
    if (v < 0) return false;
    chk = bt_polymod_step(chk, (uint32_t)v);
    if (i + 6 < n) {  // not the checksum
      acc = (acc << 5 | (uint32_t)v) & 0xFFF;
      bits += 5;
      if (bits >= 8) {
        bits -= 8;
        bytes++;
      }
    }
  }
  if (chk != 1) return false;
  if (bits >= 5 || (acc & ((1u << bits) - 1)) != 0) return false;
  return bytes >= 1 && bytes <= 255;
}

// ---- repeated fields of a MsgPayForBlobs, walked where they lie -------------------
// The elements of one repeated uint32 field of m[0, n) in order: packed spans
// and single varints mix, each value cut to 32 bits.  The buffer decoded once
// (bt_check_tx's first pass) before a cursor walks it.
struct BtU32Cursor {
  uint32_t i, in_at, in_end;
};
DAGPU_SQ_HD inline BtU32Cursor bt_u32_begin() { return BtU32Cursor{0, 0, 0}; }
DAGPU_SQ_HD inline bool bt_u32_next(const uint8_t* m, uint32_t n, uint64_t num, BtU32Cursor& c, uint32_t& v) {
  for (;;) {
    if (c.in_at < c.in_end) {
      uint64_t x;
      if (!read_varint(m, c.in_end, c.in_at, x)) return false;
      v = (uint32_t)x;
      return true;
    }
    SpField f;
    if (sp_next_field(m, n, c.i, f) <= 0) return false;
    if (f.num != num) continue;
    if (f.wt == 0) {
      v = (uint32_t)f.v;
      return true;
    }
    c.in_at = f.off;
    c.in_end = f.off + f.len;
  }
}
// element j of a repeated bytes field: its offset in m and length; false: no such element
DAGPU_SQ_HD inline bool bt_bytes_next(const uint8_t* m, uint32_t n, uint64_t num, uint32_t& i, uint32_t& off,
                                      uint32_t& len) {
  SpField f;
  while (sp_next_field(m, n, i, f) > 0)
    if (f.num == num && f.wt == 2) {
      off = f.off;
      len = f.len;
      return true;
    }
  return false;
}

// ---- the blobs of a BlobTx, walked where they lie -----------------------------------
// The next blob of tx[0, n) behind cursor i (sp_unmarshal_blob_tx's fields, its
// last-wins rule): 1, 0 at the end, -1 malformed.  Blob data is skipped by length.
DAGPU_SQ_HD inline int bt_next_blob(const uint8_t* tx, uint32_t n, uint32_t& i, SpBlobFields& b) {
  SpField f, g;
  for (;;) {
    const int st = sp_next_field(tx, n, i, f);
    if (st <= 0) return st;
    if (f.num != 2) continue;
    if (f.wt != 2) return -1;
    b.ns_off = b.ns_len = b.data_off = b.data_len = b.share_version = b.ns_version = 0;
    uint32_t j = 0;
    for (;;) {
      const int s2 = sp_next_field(tx + f.off, f.len, j, g);
      if (s2 < 0) return -1;
      if (s2 == 0) break;
      if (g.num == 1 && g.wt == 2) {
        b.ns_off = f.off + g.off;
        b.ns_len = g.len;
      } else if (g.num == 2 && g.wt == 2) {
        b.data_off = f.off + g.off;
        b.data_len = g.len;
      } else if (g.num == 3 && g.wt == 0) {
        b.share_version = (uint32_t)g.v;
      } else if (g.num == 4 && g.wt == 0) {
        b.ns_version = (uint32_t)g.v;
      }
    }
    return 1;
  }
}

// ---- one tx -------------------------------------------------------------------------
// What the tie of a plan blob to its declaration needs of a tx: whether it is a
// BlobTx, where its MsgPayForBlobs lies in it, and how many commitments it
// declares when the tx passed the commitment-length rule (0 when it failed
// before: its rows of the expected table are zero).
struct BtTxInfo {
  uint32_t is_blob_tx, pfb_off, pfb_len, ncommit;
};
DAGPU_SQ_HD inline uint32_t bt_check_tx(const uint8_t* tx, uint32_t n, BtTxInfo* info) {
  BtTxInfo t;
  t.is_blob_tx = t.pfb_off = t.pfb_len = t.ncommit = 0;
  const SpTxInfo u = sp_unmarshal_blob_tx(tx, n, 0, nullptr, 0, 0);
  t.is_blob_tx = u.is_blob_tx;
  if (info) *info = t;
  BtMsgs msgs;
  if (!u.is_blob_tx) {
    if (!bt_walk_msgs(tx, n, msgs) || msgs.first_pfb == kBtNone) return kBtOk;
    return bt_word(kBtNonBlobTxHasPfb, msgs.first_pfb);
  }
  const uint8_t* inner = tx + u.inner_off;
  if (!bt_walk_msgs(inner, u.inner_len, msgs)) return kBtDecode;
  if (msgs.count != 1) return bt_word(kBtMultipleMsgs, msgs.count);
  if (msgs.first_pfb != 0) return kBtNoPfb;
  const uint8_t* m = inner + msgs.val_off;
  const uint32_t mn = msgs.val_len;

  // one pass over the message: the counts, the signer, the first fault of each
  // per-element rule
  uint32_t n_ns = 0, n_sz = 0, n_cm = 0, n_sv = 0, signer_off = 0, signer_len = 0;
  uint32_t ns_fault = 0, ns_at = 0, sv_at = kBtNone, cm_at = kBtNone;
  {
    uint32_t i = 0;
    SpField f;
    for (;;) {
      const int st = sp_next_field(m, mn, i, f);
      if (st < 0) return kBtPfbDecode;
      if (st == 0) break;
      if (f.num == 1) {
        if (f.wt != 2) return kBtPfbDecode;
        signer_off = f.off;
        signer_len = f.len;
      } else if (f.num == 2) {
        if (f.wt != 2) return kBtPfbDecode;
        if (!ns_fault) {
          const uint8_t* p = m + f.off;
          ns_fault = f.len != kBtNsSize ? 1 : bt_namespace_rule([p](uint32_t q) { return p[q]; });
          ns_at = n_ns;
        }
        n_ns++;
      } else if (f.num == 4) {
        if (f.wt != 2) return kBtPfbDecode;
        if (cm_at == kBtNone && f.len != kBtCommitment) cm_at = n_cm;
        n_cm++;
      } else if (f.num == 3 || f.num == 8) {
        if (f.wt != 0 && f.wt != 2) return kBtPfbDecode;
        uint32_t at = f.off;
        const uint32_t end = f.off + f.len;
        do {
          uint64_t v = f.v;
          if (f.wt == 2) {
            if (at >= end) break;
            if (!read_varint(m, end, at, v)) return kBtPfbDecode;
          }
          if (f.num == 3) {
            n_sz++;
          } else {
            if (sv_at == kBtNone && (uint32_t)v != 0) sv_at = n_sv;
            n_sv++;
          }
        } while (f.wt == 2);
      }
    }
  }
  if (n_ns == 0) return kBtNoNamespaces;
  if (n_sv == 0) return kBtNoShareVersions;
  if (n_sz == 0) return kBtNoBlobSizes;
  if (n_cm == 0) return kBtNoShareCommitments;
  if (n_ns != n_sv || n_ns != n_sz || n_ns != n_cm) return kBtMismatchedCounts;
  if (ns_fault)
    return bt_word(ns_fault == 1 ? kBtInvalidNamespace : ns_fault == 2 ? kBtReservedNamespace : kBtInvalidNamespaceVersion,
                   ns_at);
  if (sv_at != kBtNone) return bt_word(kBtUnsupportedShareVersion, sv_at);
  if (!bt_signer_ok(m + signer_off, signer_len)) return kBtBadSigner;
  if (cm_at != kBtNone) return bt_word(kBtBadCommitmentLength, cm_at);
  t.pfb_off = u.inner_off + msgs.val_off;
  t.pfb_len = mn;
  t.ncommit = n_cm;
  if (info) *info = t;

  // ValidateBlobs
  SpBlobFields b;
  uint32_t at = 0, j = 0;
  while (bt_next_blob(tx, n, at, b) > 0) {
    if (b.ns_version > 255) return bt_word(kBtBlobNsVersionTooLarge, j);
    const uint8_t* id = tx + b.ns_off;  // 28 bytes: the tx is a BlobTx
    const uint8_t version = (uint8_t)b.ns_version;
    const uint32_t rule = bt_namespace_rule([id, version](uint32_t q) { return q == 0 ? version : id[q - 1]; });
    if (rule) return bt_word(kBtBlobInvalidNamespace + rule - 1, j);
    if (b.data_len == 0) return bt_word(kBtZeroBlobSize, j);
    if ((uint8_t)b.share_version != 0) return bt_word(kBtBlobUnsupportedShareVersion, j);
    j++;
  }
  // the sizes, then the namespaces, of blob j against declaration j
  if (u.nblob != n_sz) return bt_word(kBtSizeMismatch, u.nblob < n_sz ? u.nblob : n_sz);
  BtU32Cursor sizes = bt_u32_begin();
  at = 0;
  for (j = 0; j < u.nblob; j++) {
    uint32_t declared = 0;
    if (bt_next_blob(tx, n, at, b) <= 0 || !bt_u32_next(m, mn, 3, sizes, declared)) return kBtDecode;  // walked before: not reached
    if (b.data_len != declared) return bt_word(kBtSizeMismatch, j);
  }
  uint32_t ns_i = 0;
  at = 0;
  for (j = 0; j < u.nblob; j++) {
    uint32_t off = 0, len = 0;
    if (bt_next_blob(tx, n, at, b) <= 0 || !bt_bytes_next(m, mn, 2, ns_i, off, len)) return kBtDecode;  // as above
    const uint8_t* id = tx + b.ns_off;
    bool same = m[off] == (uint8_t)b.ns_version;
    for (uint32_t q = 0; q < kSpNsId; q++) same = same && m[off + 1 + q] == id[q];
    if (!same) return bt_word(kBtNamespaceMismatch, j);
  }
  return kBtOk;
}

// ---- a batch: tables, the per-tx step and the tie of a plan blob ----------------------
// workspace: lowest[n] (uint64) | SpBlockIn[n] | SpTxIn[ntx] | blob_base[n + 1] | BtTxInfo[ntx]
struct BtCarve {
  uint64_t blk, tx, base, info, total;
};
DAGPU_SQ_HD inline BtCarve bt_carve(uint64_t n, uint64_t ntx) {
  BtCarve c;
  c.blk = sp_up16(n * 8);
  c.tx = c.blk + n * sizeof(SpBlockIn);
  c.base = c.tx + ntx * sizeof(SpTxIn);
  c.info = sp_up16(c.base + (n + 1) * 8);
  c.total = c.info + ntx * sizeof(BtTxInfo);
  return c;
}
struct BtArgs {
  const uint8_t* src;
  const SpBlockIn* blk;
  const SpTxIn* tx;
  const uint64_t* blob_base;  // n + 1
  BtTxInfo* info;
  unsigned long long* lowest;  // per block: tx index << 32 | word of the lowest failing tx
  const uint8_t* arena;
  uint64_t arena_cap;
  const SpRecord* rec;
  uint32_t* tx_status;
  uint32_t* block_status;
  uint8_t* expected;
  uint32_t n;
  uint64_t ntx_total, nrows;
};
static_assert(sizeof(BtTxInfo) == 16 && sizeof(SpTxIn) == 16, "validation tables");

// tx g of the batch: its word and its BtTxInfo; the caller folds the word into
// its block's lowest (the returned key), by an atomic min or a plain one
DAGPU_SQ_HD inline uint64_t bt_validate_tx(const BtArgs& a, uint64_t g, uint32_t& blk) {
  const SpTxIn t = a.tx[g];
  blk = t.blk;
  const SpBlockIn b = a.blk[t.blk];
  BtTxInfo info;
  const uint32_t word = bt_check_tx(a.src + b.src_off + t.off, t.len, &info);
  a.info[g] = info;
  a.tx_status[g] = word;
  return word ? ((uint64_t)((uint32_t)g - b.tx_base) << 32 | word) : ~(uint64_t)0;
}
// block i's two words from its lowest key
DAGPU_SQ_HD inline void bt_finish_block(const BtArgs& a, uint32_t i) {
  const uint64_t key = a.lowest[i];
  a.block_status[2 * i] = (uint32_t)(key >> 32);
  a.block_status[2 * i + 1] = key == ~(uint64_t)0 ? 0 : (uint32_t)key;
}
// Row `row` of the expected table: the block that owns it (binary search over
// blob_base), the plan blob's data_off, the tx that holds that offset (binary
// search over the block's tx offsets), the blob of that tx whose data lies
// there (a walk of the one tx), and that blob's declared commitment.  Anything
// that does not tie (a block without a plan, a row past the plan's blobs, a tx
// that failed before its commitment lengths were checked) leaves zeros.
// `owner` (null, or two words per row) receives the block-local index of the tx
// that owns the blob and the blob's index inside that tx, or kBtNone twice for
// a row that does not tie.
DAGPU_SQ_HD inline void bt_tie_row(const BtArgs& a, uint64_t row, uint32_t* owner = nullptr) {
  uint32_t lo = 0, hi = a.n;  // the last block with blob_base <= row
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a.blob_base[mid] <= row) lo = mid;
    else hi = mid;
  }
  const SpBlockIn b = a.blk[lo];
  const SpRecord r = a.rec[lo];
  const uint64_t i = row - a.blob_base[lo];
  uint32_t from = kBtNone;  // of the 32 bytes, in src
  uint32_t own_tx = kBtNone, own_blob = kBtNone;
  const uint8_t* src = a.src + b.src_off;
  do {
    if (r.plan_bytes < sizeof(SqHdr) || r.plan_off > a.arena_cap || r.plan_bytes > a.arena_cap - r.plan_off)
      break;
    const SqHdr* h = (const SqHdr*)(a.arena + r.plan_off);
    if (i >= h->nblob || h->blob_off > r.plan_bytes ||
        (uint64_t)h->nblob * kSqBlobWords * 4 > r.plan_bytes - h->blob_off)
      break;
    const uint32_t data_off = ((const uint32_t*)(a.arena + r.plan_off + h->blob_off))[i * kSqBlobWords + 10];
    if (b.ntx == 0 || data_off >= b.src_len) break;
    uint32_t tl = 0, th = b.ntx;  // the last tx with off <= data_off
    while (th - tl > 1) {
      const uint32_t mid = tl + ((th - tl) >> 1);
      if (a.tx[b.tx_base + mid].off <= data_off) tl = mid;
      else th = mid;
    }
    const SpTxIn t = a.tx[b.tx_base + tl];
    const BtTxInfo info = a.info[b.tx_base + tl];
    if (!info.is_blob_tx || info.ncommit == 0 || data_off < t.off || data_off - t.off >= t.len) break;
    const uint8_t* tx = src + t.off;
    SpBlobFields f;
    uint32_t at = 0, j = 0;
    bool found = false;
    while (bt_next_blob(tx, t.len, at, f) > 0) {
      if (f.data_len && f.data_off == data_off - t.off) {
        found = true;
        break;
      }
      j++;
    }
    if (!found || j >= info.ncommit) break;
    uint32_t ci = 0, off = 0, len = 0;
    bool have = false;
    for (uint32_t q = 0; q <= j; q++) have = bt_bytes_next(tx + info.pfb_off, info.pfb_len, 4, ci, off, len);
    if (!have || len != kBtCommitment) break;
    from = t.off + info.pfb_off + off;
    own_tx = tl;
    own_blob = j;
  } while (false);
  if (owner) {
    owner[2 * row] = own_tx;
    owner[2 * row + 1] = own_blob;
  }
  uint8_t* out = a.expected + row * kBtCommitment;
  for (uint32_t q = 0; q < kBtCommitment; q++) out[q] = from == kBtNone ? (uint8_t)0 : src[from + q];
}

inline BtArgs bt_args(uint8_t* ws, const uint8_t* src, uint64_t n, uint64_t ntx_total, uint64_t nrows,
                      const uint8_t* plans, uint64_t plans_cap, const void* records, uint32_t* tx_status,
                      uint32_t* block_status, uint8_t* expected) {
  const BtCarve c = bt_carve(n, ntx_total);
  BtArgs a;
  a.src = src;
  a.blk = (const SpBlockIn*)(ws + c.blk);
  a.tx = (const SpTxIn*)(ws + c.tx);
  a.blob_base = (const uint64_t*)(ws + c.base);
  a.info = (BtTxInfo*)(ws + c.info);
  a.lowest = (unsigned long long*)ws;
  a.arena = plans;
  a.arena_cap = plans_cap;
  a.rec = (const SpRecord*)records;
  a.tx_status = tx_status;
  a.block_status = block_status;
  a.expected = expected;
  a.n = (uint32_t)n;
  a.ntx_total = ntx_total;
  a.nrows = nrows;
  return a;
}

// blobtx_host.cpp: the checks of one call, before anything is enqueued, and
// its upload: sp_tables' SpBlockIn[n] | SpTxIn[ntx], then blob_base[n + 1]
// (zeros for a null blob_base: no rows).  ctx may be null (the host executor).
int bt_request(dagpu_ctx* ctx, size_t n, const void* src, const size_t* src_offs, size_t src_bytes, const uint32_t* ntx,
               const uint64_t* tx_lens, const void* plans, const void* records, const uint64_t* blob_base,
               const void* tx_status, const void* block_status, const void* expected, std::vector<uint8_t>& up,
               uint64_t& ntx_total, uint64_t& nrows);

}  // namespace dagpu
