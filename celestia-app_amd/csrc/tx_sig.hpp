// tx_sig.hpp -- the stateless half of the SigVerificationDecorator
// (app/ante/ante.go:55, reached from app/process_proposal.go:103 and :126;
// cosmos-sdk v0.46 x/auth/ante/sigverify.go) over the txs of a batch where they
// lie: one secp256k1 ECDSA verification over SHA-256(SignDoc) per tx, in one
// copy for the host (tx_sig_host.cpp) and the device (tx_sig.hip).  The
// stateful inputs (account numbers, stored public keys) come in as tables.
//
// ts_walk_tx, per tx: a BlobTx is unwrapped to its inner tx (sp_unmarshal_blob_tx);
// then Tx {body_bytes 1, auth_info_bytes 2, signatures 3} -> AuthInfo
// {signer_infos 1} -> SignerInfo {public_key 1 (Any), mode_info 2, sequence 3}
// -> ModeInfo {single 1 {mode 1}, multi 2} and Any {type_url 1, value 2} ->
// PubKey {key 1}.  It is the project's walker (sp_next_field, bt_walk_msgs:
// unknown fields skipped, the last of a field wins, a wrong wire type on a
// field it reads or a malformed buffer fails); the SDK's stricter
// canonical-encoding rejections (unknown fields, non-minimal varints, field
// order) are not restated.  body_bytes and auth_info_bytes are the exact byte
// ranges of fields 1 and 2, as the SDK's decoder keeps them.  The first that
// applies (a word is kind | index << 8):
//   kSigTxUndecodable       the walk fails, the body's messages included
//   kSigUnsupportedSigners  signer_infos or signatures count != 1; index = the
//                           signer_infos count
//   kSigUnsupportedMode     not Single {SIGN_MODE_DIRECT = 1}; index = the mode
//                           (its low 32 bits, as the int32 enum takes them), 0
//                           for Multi or no mode_info
//   kSigUnsupportedPubkeyType  a public_key of another type_url
//   (kSigTxUndecodable      the PubKey value does not decode)
//   kSigNoPubkey            no public_key in the tx (and no row in the table)
//   kSigBadPubkey           the key is not 33 bytes (the curve checks follow in
//                           secp_verify)
//   kSigBadLength           the signature is not 64 bytes; index = its length
// The walker alone (no table) gives the signer record's kind; with a table row
// (first byte != 0) that row is the key, as the account's stored key is in the
// reference, and the tx's own key is not looked at beyond its type.
//
// ts_sign_doc_hash streams DirectSignBytes into SHA-256 without materialising
// it: SignDoc {body_bytes 1, auth_info_bytes 2, chain_id 3, account_number 4},
// a field omitted when empty or 0, then the padding, through one put() site.
// The sink S keeps the 16-word block (LDS on the device, tx_sig.hip; a plain
// buffer on the host).  No byte at or past a tx's n is read.
#pragma once
#include <stdint.h>

#include "blobtx_check.hpp"
#include "host_sha256.hpp"
#include "secp256k1.hpp"

namespace dagpu {

constexpr uint32_t kTsRecord = 136;  // z[32] r[32] s[32] pubkey[33] pad[7]
constexpr uint32_t kTsSigner = 48;   // pubkey[33] kind u8 pad[6] sequence u64
constexpr uint32_t kTsMaxChainId = 64;
constexpr uint32_t kTsKeyUrlLen = 31;

struct TsTx {
  uint32_t kind, index;  // the walker's own classification, no table
  uint32_t body_off, body_len, auth_off, auth_len, sig_off, sig_len;  // from the start of the tx
  uint32_t has_key, key_off, key_len;
  uint64_t sequence;
};

DAGPU_SQ_HD inline bool ts_is_key_url(const uint8_t* p, uint32_t len) {
  const char* url = "/cosmos.crypto.secp256k1.PubKey";
  if (len != kTsKeyUrlLen) return false;
  for (uint32_t i = 0; i < kTsKeyUrlLen; i++)
    if (p[i] != (uint8_t)url[i]) return false;
  return true;
}

DAGPU_SQ_HD inline void ts_fail(TsTx& t, uint32_t kind, uint64_t index) {
  t.kind = kind;
  t.index = (uint32_t)(index > 0xFFFFFFu ? 0xFFFFFFu : index);
  if (kind == kSigTxUndecodable || kind == kSigUnsupportedSigners) t.sequence = 0;
}

DAGPU_SQ_HD inline void ts_walk_tx(const uint8_t* tx, uint32_t n, TsTx& t) {
  t.kind = t.index = t.body_off = t.body_len = t.auth_off = t.auth_len = t.sig_off = t.sig_len = 0;
  t.has_key = t.key_off = t.key_len = 0;
  t.sequence = 0;
  const SpTxInfo u = sp_unmarshal_blob_tx(tx, n, 0, nullptr, 0, 0);
  const uint32_t base = u.is_blob_tx ? u.inner_off : 0, len = u.is_blob_tx ? u.inner_len : n;
  const uint8_t* b = tx + base;
  SpField f;
  uint32_t i = 0, nsig = 0;
  for (;;) {
    const int st = sp_next_field(b, len, i, f);
    if (st < 0) return ts_fail(t, kSigTxUndecodable, 0);
    if (st == 0) break;
    if (f.num < 1 || f.num > 3) continue;
    if (f.wt != 2) return ts_fail(t, kSigTxUndecodable, 0);
    if (f.num == 1) {
      t.body_off = base + f.off;
      t.body_len = f.len;
    } else if (f.num == 2) {
      t.auth_off = base + f.off;
      t.auth_len = f.len;
    } else {
      if (nsig == 0) {
        t.sig_off = base + f.off;
        t.sig_len = f.len;
      }
      nsig++;
    }
  }
  BtMsgs msgs;
  if (!bt_walk_msgs(b, len, msgs)) return ts_fail(t, kSigTxUndecodable, 0);
  // AuthInfo
  uint32_t nsi = 0, si_off = 0, si_len = 0;
  i = 0;
  for (;;) {
    const int st = sp_next_field(tx + t.auth_off, t.auth_len, i, f);
    if (st < 0) return ts_fail(t, kSigTxUndecodable, 0);
    if (st == 0) break;
    if (f.num != 1) continue;
    if (f.wt != 2) return ts_fail(t, kSigTxUndecodable, 0);
    if (nsi == 0) {
      si_off = t.auth_off + f.off;
      si_len = f.len;
    }
    nsi++;
  }
  if (nsi != 1 || nsig != 1) return ts_fail(t, kSigUnsupportedSigners, nsi);
  // SignerInfo
  uint32_t has_pk = 0, pk_off = 0, pk_len = 0, mi_off = 0, mi_len = 0;
  i = 0;
  for (;;) {
    const int st = sp_next_field(tx + si_off, si_len, i, f);
    if (st < 0) return ts_fail(t, kSigTxUndecodable, 0);
    if (st == 0) break;
    if (f.num == 1) {
      if (f.wt != 2) return ts_fail(t, kSigTxUndecodable, 0);
      has_pk = 1;
      pk_off = si_off + f.off;
      pk_len = f.len;
    } else if (f.num == 2) {
      if (f.wt != 2) return ts_fail(t, kSigTxUndecodable, 0);
      mi_off = si_off + f.off;
      mi_len = f.len;
    } else if (f.num == 3) {
      if (f.wt != 0) return ts_fail(t, kSigTxUndecodable, 0);
      t.sequence = f.v;
    }
  }
  // ModeInfo: a oneof, the last member wins
  uint32_t which = 0, single_off = 0, single_len = 0, mode = 0;
  i = 0;
  for (;;) {
    const int st = sp_next_field(tx + mi_off, mi_len, i, f);
    if (st < 0) return ts_fail(t, kSigTxUndecodable, 0);
    if (st == 0) break;
    if (f.num != 1 && f.num != 2) continue;
    if (f.wt != 2) return ts_fail(t, kSigTxUndecodable, 0);
    which = (uint32_t)f.num;
    if (f.num == 1) {
      single_off = mi_off + f.off;
      single_len = f.len;
    }
  }
  if (which == 1) {
    i = 0;
    for (;;) {
      const int st = sp_next_field(tx + single_off, single_len, i, f);
      if (st < 0) return ts_fail(t, kSigTxUndecodable, 0);
      if (st == 0) break;
      if (f.num != 1) continue;
      if (f.wt != 0) return ts_fail(t, kSigTxUndecodable, 0);
      mode = (uint32_t)f.v;
    }
  }
  // Any
  uint32_t url_off = 0, url_len = 0, val_off = 0, val_len = 0;
  if (has_pk) {
    i = 0;
    for (;;) {
      const int st = sp_next_field(tx + pk_off, pk_len, i, f);
      if (st < 0) return ts_fail(t, kSigTxUndecodable, 0);
      if (st == 0) break;
      if (f.num != 1 && f.num != 2) continue;
      if (f.wt != 2) return ts_fail(t, kSigTxUndecodable, 0);
      if (f.num == 1) {
        url_off = pk_off + f.off;
        url_len = f.len;
      } else {
        val_off = pk_off + f.off;
        val_len = f.len;
      }
    }
  }
  if (which != 1) return ts_fail(t, kSigUnsupportedMode, 0);
  if (mode != 1) return ts_fail(t, kSigUnsupportedMode, mode);
  if (has_pk) {
    if (!ts_is_key_url(tx + url_off, url_len)) return ts_fail(t, kSigUnsupportedPubkeyType, 0);
    i = 0;
    for (;;) {
      const int st = sp_next_field(tx + val_off, val_len, i, f);
      if (st < 0) return ts_fail(t, kSigTxUndecodable, 0);
      if (st == 0) break;
      if (f.num != 1) continue;
      if (f.wt != 2) return ts_fail(t, kSigTxUndecodable, 0);
      t.key_off = val_off + f.off;
      t.key_len = f.len;
    }
    t.has_key = 1;
  }
  if (!t.has_key) return ts_fail(t, kSigNoPubkey, 0);
  if (t.key_len != 33) return ts_fail(t, kSigBadPubkey, 0);
  if (t.sig_len != 64) return ts_fail(t, kSigBadLength, t.sig_len);
}

// the word of a tx before any curve arithmetic, given whether the table has a key for it
DAGPU_SQ_HD inline uint32_t ts_pre_word(const TsTx& t, bool table_key) {
  if (t.kind >= kSigTxUndecodable && t.kind <= kSigUnsupportedPubkeyType) return bt_word(t.kind, t.index);
  if (!table_key) {
    if (!t.has_key) return kSigNoPubkey;
    if (t.key_len != 33) return kSigBadPubkey;
  }
  if (t.sig_len != 64) return bt_word(kSigBadLength, t.sig_len);
  return kSigOk;
}

// ---- DirectSignBytes into SHA-256 -------------------------------------------------------
// tag, then v as a varint: at most 11 bytes, byte j at bits 8 j of lo (j < 8) or 8 (j - 8) of hi
DAGPU_SQ_HD inline uint32_t ts_header(uint8_t tag, uint64_t v, uint64_t& lo, uint64_t& hi) {
  lo = tag;
  hi = 0;
  uint32_t n = 1;
  do {
    uint64_t b = v & 0x7F;
    v >>= 7;
    if (v) b |= 0x80;
    if (n < 8) lo |= b << (8 * n);
    else hi |= b << (8 * (n - 8));
    n++;
  } while (v);
  return n;
}
struct TsSeg {
  uint64_t lo, hi;
  uint32_t hlen, dlen;
  const uint8_t* p;
};
// field `seg` (0 .. 3) of the SignDoc; hlen = 0: omitted
DAGPU_SQ_HD inline TsSeg ts_segment(uint32_t seg, const uint8_t* body, uint32_t body_len, const uint8_t* auth,
                                    uint32_t auth_len, const uint8_t* chain, uint32_t chain_len, uint64_t acct) {
  TsSeg s;
  s.p = seg == 0 ? body : seg == 1 ? auth : chain;
  s.dlen = seg == 0 ? body_len : seg == 1 ? auth_len : seg == 2 ? chain_len : 0;
  const uint64_t v = seg == 3 ? acct : s.dlen;
  s.hlen = ts_header((uint8_t)((seg + 1) << 3 | (seg == 3 ? 0 : 2)), v, s.lo, s.hi);
  if (v == 0) s.hlen = s.dlen = 0;
  return s;
}
// S: put(byte) and finish(out32)
template <class S>
DAGPU_SQ_HD DAGPU_EC_INLINE void ts_sign_doc_hash(S& sink, const uint8_t* body, uint32_t body_len, const uint8_t* auth,
                                                  uint32_t auth_len, const uint8_t* chain, uint32_t chain_len,
                                                  uint64_t acct, uint8_t* out32) {
  uint64_t total = 0;
  for (uint32_t seg = 0; seg < 4; seg++) {
    const TsSeg s = ts_segment(seg, body, body_len, auth, auth_len, chain, chain_len, acct);
    total += (uint64_t)s.hlen + s.dlen;
  }
  const uint32_t npad = ((55u - (uint32_t)(total & 63)) & 63) + 1;  // 0x80 and zeros up to 56 mod 64
  const uint64_t bits = total * 8;
#pragma unroll 1
  for (uint32_t seg = 0; seg < 5; seg++) {
    TsSeg s;
    uint64_t count;
    if (seg < 4) {
      s = ts_segment(seg, body, body_len, auth, auth_len, chain, chain_len, acct);
      count = (uint64_t)s.hlen + s.dlen;
    } else {
      s.lo = s.hi = 0;
      s.hlen = s.dlen = 0;
      s.p = nullptr;
      count = npad + 8;
    }
#pragma unroll 1
    for (uint64_t j = 0; j < count; j++) {
      uint8_t b;
      if (seg < 4) {
        if (j < s.hlen) b = (uint8_t)(j < 8 ? s.lo >> (8 * j) : s.hi >> (8 * (j - 8)));
        else b = s.p[j - s.hlen];
      } else {
        b = j == 0 ? (uint8_t)0x80 : j < npad ? (uint8_t)0 : (uint8_t)(bits >> (8 * (7 - (j - npad))));
      }
      sink.put(b);
    }
  }
  sink.finish(out32);
}

// ---- a batch ---------------------------------------------------------------------------
// workspace: lowest[n] (uint64) | not_judged[n] | SpBlockIn[n] | SpTxIn[ntx] | chain id[64] | records[ntx]
struct TsCarve {
  uint64_t nj, blk, tx, chain, rec, total;
};
DAGPU_SQ_HD inline TsCarve ts_carve(uint64_t n, uint64_t ntx) {
  TsCarve c;
  c.nj = sp_up16(n * 8);
  c.blk = c.nj + sp_up16(n * 4);
  c.tx = c.blk + n * sizeof(SpBlockIn);
  c.chain = c.tx + ntx * sizeof(SpTxIn);
  c.rec = c.chain + kTsMaxChainId;
  c.total = c.rec + ntx * kTsRecord;
  return c;
}
struct TsArgs {
  const uint8_t* src;
  const SpBlockIn* blk;
  const SpTxIn* tx;
  const uint8_t* chain;
  const uint64_t* acct;
  const uint8_t* pubkeys;  // may be null
  uint8_t* rec;            // null: signer records only
  uint8_t* signers;
  uint32_t* tx_status;
  uint32_t* block_status;
  unsigned long long* lowest;
  uint32_t* not_judged;
  uint32_t n, chain_len;
  uint64_t ntx_total;
};
// what the verification lanes read: the records above, or the three arrays of
// dagpu_secp256k1_verify_* (raw: no word comes in, nothing is folded)
struct TsVerifyArgs {
  const uint8_t *z, *sig, *pk;
  uint32_t z_stride, sig_stride, pk_stride, raw;
  uint32_t* status;
  uint64_t count;
  const SpBlockIn* blk;
  const SpTxIn* tx;
  unsigned long long* lowest;
  uint32_t* not_judged;
};

DAGPU_SQ_HD inline void ts_put_signer(uint8_t* out, const uint8_t* tx, const TsTx& t) {
  const bool key = t.has_key && t.key_len == 33;
  for (uint32_t q = 0; q < 33; q++) out[q] = key ? tx[t.key_off + q] : (uint8_t)0;
  out[33] = (uint8_t)t.kind;
  for (uint32_t q = 34; q < 40; q++) out[q] = 0;
  for (uint32_t q = 0; q < 8; q++) out[40 + q] = (uint8_t)(t.sequence >> (8 * q));
}

// tx g of the batch: its signer record, and with a.rec its word before the
// curve arithmetic and (word 0 or kSigBadLength) its verification record
template <class S>
DAGPU_SQ_HD DAGPU_EC_INLINE void ts_prepare_tx(const TsArgs& a, uint64_t g, S& sink) {
  const SpTxIn ti = a.tx[g];
  const uint8_t* tx = a.src + a.blk[ti.blk].src_off + ti.off;
  TsTx t;
  ts_walk_tx(tx, ti.len, t);
  ts_put_signer(a.signers + g * kTsSigner, tx, t);
  if (!a.rec) return;
  const uint8_t* row = a.pubkeys ? a.pubkeys + g * 33 : nullptr;
  const bool table_key = row && row[0] != 0;
  const uint32_t word = ts_pre_word(t, table_key);
  a.tx_status[g] = word;
  const uint32_t kind = word & 0xFF;
  if (kind != kSigOk && kind != kSigBadLength) return;
  uint8_t* rec = a.rec + g * kTsRecord;
  const uint8_t* key = table_key ? row : tx + t.key_off;
  for (uint32_t q = 0; q < 33; q++) rec[96 + q] = key[q];
  if (kind != kSigOk) return;
  for (uint32_t q = 0; q < 64; q++) rec[32 + q] = tx[t.sig_off + q];
  ts_sign_doc_hash(sink, tx + t.body_off, t.body_len, tx + t.auth_off, t.auth_len, a.chain, a.chain_len, a.acct[g],
                   rec);
}

// item g: the curve arithmetic and the final word; the returned key folds into
// the block's lowest (all ones: nothing to fold), *not_judged says whether the
// tx counts as not judged
DAGPU_SQ_HD DAGPU_EC_INLINE uint64_t ts_verify_item(const TsVerifyArgs& a, uint64_t g, uint32_t& blk,
                                                    bool& not_judged) {
  const uint8_t* z = a.z + g * a.z_stride;
  const uint8_t* sig = a.sig + g * a.sig_stride;
  const uint8_t* pk = a.pk + g * a.pk_stride;
  not_judged = false;
  blk = 0;
  // one copy of the curve arithmetic for both callers: a raw item comes in as word 0
  uint32_t word = a.raw ? (uint32_t)kSigOk : a.status[g];
  const uint32_t kind = word & 0xFF;
  if (kind == kSigOk || kind == kSigBadLength) {
    U256 qx, qy;
    if (!secp_parse_pubkey(pk, qx, qy)) word = kSigBadPubkey;
    else if (kind == kSigOk) word = secp_verify_point(z, sig, sig + 32, qx, qy);
    a.status[g] = word;
  }
  if (a.raw) return ~(uint64_t)0;
  const SpTxIn ti = a.tx[g];
  blk = ti.blk;
  if ((word & 0xFF) >= kSigBadPubkey) return (uint64_t)((uint32_t)g - a.blk[ti.blk].tx_base) << 32 | word;
  not_judged = (word & 0xFF) != kSigOk;
  return ~(uint64_t)0;
}
// block i's four words
DAGPU_SQ_HD inline void ts_finish_block(const TsArgs& a, uint32_t i) {
  const uint64_t key = a.lowest[i];
  a.block_status[4 * i] = (uint32_t)(key >> 32);
  a.block_status[4 * i + 1] = key == ~(uint64_t)0 ? 0 : (uint32_t)key;
  a.block_status[4 * i + 2] = a.not_judged[i];
  a.block_status[4 * i + 3] = 0;
}

inline TsArgs ts_args(uint8_t* ws, const uint8_t* src, uint64_t n, uint64_t ntx_total, uint32_t chain_len,
                      const uint64_t* acct, const uint8_t* pubkeys, bool verify, uint8_t* signers,
                      uint32_t* tx_status, uint32_t* block_status) {
  const TsCarve c = ts_carve(n, ntx_total);
  TsArgs a;
  a.src = src;
  a.blk = (const SpBlockIn*)(ws + c.blk);
  a.tx = (const SpTxIn*)(ws + c.tx);
  a.chain = ws + c.chain;
  a.acct = acct;
  a.pubkeys = pubkeys;
  a.rec = verify ? ws + c.rec : nullptr;
  a.signers = signers;
  a.tx_status = tx_status;
  a.block_status = block_status;
  a.lowest = (unsigned long long*)ws;
  a.not_judged = (uint32_t*)(ws + c.nj);
  a.n = (uint32_t)n;
  a.chain_len = chain_len;
  a.ntx_total = ntx_total;
  return a;
}
inline TsVerifyArgs ts_verify_args(const TsArgs& a) {
  TsVerifyArgs v;
  v.z = a.rec;
  v.sig = a.rec + 32;
  v.pk = a.rec + 96;
  v.z_stride = v.sig_stride = v.pk_stride = kTsRecord;
  v.raw = 0;
  v.status = a.tx_status;
  v.count = a.ntx_total;
  v.blk = a.blk;
  v.tx = a.tx;
  v.lowest = a.lowest;
  v.not_judged = a.not_judged;
  return v;
}
inline TsVerifyArgs ts_raw_args(uint64_t count, const uint8_t* digests, const uint8_t* sigs, const uint8_t* pubkeys,
                                uint32_t* status) {
  TsVerifyArgs v;
  v.z = digests;
  v.sig = sigs;
  v.pk = pubkeys;
  v.z_stride = 32;
  v.sig_stride = 64;
  v.pk_stride = 33;
  v.raw = 1;
  v.status = status;
  v.count = count;
  v.blk = nullptr;
  v.tx = nullptr;
  v.lowest = nullptr;
  v.not_judged = nullptr;
  return v;
}

// ---- the executors as host loops ----------------------------------------------------------
// What dagpu_tx_sig_verify_host / dagpu_tx_signers_host and
// dagpu_secp256k1_verify_host run behind their request checks
// (tests/host/tx_sig_check.cpp runs the same loops under the sanitizers).
// ts_sign_doc_hash's sink on the host: the block in a plain buffer.
struct TsHostSha {
  host::Sha256 s;
  uint8_t buf[64];
  uint32_t at = 0;
  void put(uint8_t b) {
    buf[at++] = b;
    if (at == 64) {
      s.block(buf);
      at = 0;
    }
  }
  void finish(uint8_t* out) {
    for (int i = 0; i < 8; i++) {
      out[4 * i] = (uint8_t)(s.h[i] >> 24);
      out[4 * i + 1] = (uint8_t)(s.h[i] >> 16);
      out[4 * i + 2] = (uint8_t)(s.h[i] >> 8);
      out[4 * i + 3] = (uint8_t)s.h[i];
    }
  }
};
// a.lowest all ones and a.not_judged zero on entry
inline void ts_run_host(const TsArgs& a) {
  for (uint64_t g = 0; g < a.ntx_total; g++) {
    TsHostSha sink;
    ts_prepare_tx(a, g, sink);
  }
  if (!a.rec) return;
  const TsVerifyArgs v = ts_verify_args(a);
  for (uint64_t g = 0; g < a.ntx_total; g++) {
    uint32_t blk;
    bool nj;
    const uint64_t key = ts_verify_item(v, g, blk, nj);
    if (key < a.lowest[blk]) a.lowest[blk] = key;
    if (nj) a.not_judged[blk]++;
  }
  for (uint32_t i = 0; i < a.n; i++) ts_finish_block(a, i);
}
inline void ts_run_raw_host(const TsVerifyArgs& v) {
  for (uint64_t g = 0; g < v.count; g++) {
    uint32_t blk;
    bool nj;
    ts_verify_item(v, g, blk, nj);
  }
}

// tx_sig_host.cpp: the checks of one call, before anything is enqueued, and
// its upload: sp_tables' SpBlockIn[n] | SpTxIn[ntx], then the chain id in 64
// bytes.  ctx may be null (the host executors).
int ts_request(dagpu_ctx* ctx, size_t n, const void* src, const size_t* src_offs, size_t src_bytes, const uint32_t* ntx,
               const uint64_t* tx_lens, bool verify, const uint8_t* chain_id, size_t chain_id_len,
               const void* account_numbers, const void* tx_status, const void* block_status, const void* signers,
               std::vector<uint8_t>& up, uint64_t& ntx_total);

}  // namespace dagpu
