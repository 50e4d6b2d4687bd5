// square.cpp -- original data square construction on the host side of the C
// ABI: the txs -> ODS step of block replay, before the GPU
// extends the square (app/extend_block.go:14-22: square.Construct then
// da.ExtendShares).  Byte bookkeeping, no device code.
//
// Restates, for app version 1 (SquareSizeUpperBound 128, SubtreeRootThreshold 64):
//   square.Construct / square.Build         pkg/square/square.go:22-63
//   Builder (AppendTx, AppendBlobTx, Export) pkg/square/builder.go
//   WriteSquare                             pkg/square/square.go
//   CompactShareCounter                     pkg/shares/counter.go
//   CompactShareSplitter                    pkg/shares/split_compact_shares.go
//   SparseShareSplitter                     pkg/shares/split_sparse_shares.go
//   Builder (share)                         pkg/shares/share_builder.go
//   padding shares                          pkg/shares/padding.go
//   blob.UnmarshalBlobTx                    pkg/blob/blob.go:56-90 (gogoproto wire format)
//   IndexWrapper marshal                    celestia-core proto/tendermint/types (type_id "INDX")
//   inclusion.SubTreeWidth / NextShareIndex pkg/inclusion/blob_share_commitment_rules.go
// with the error texts of the Python mirror (celestia_da/square.py,
// shares.py), which tests/test_square_native.py compares byte for byte.
// Shares are written straight into the caller's ODS buffer: no per-share
// allocation (the Python mirror takes ~0.17 s per full 128 x 128 square).
//
// The layout (SquareBuilder::layout: where every run of shares starts, with
// every check) is separate from the writing, so the same layout also comes out
// as a plan (dagpu_square_plan; format and per-share writer in
// square_write.hpp) that dagpu_square_plan_write_host or the kernel of
// square_write.hip turn into the same bytes from the caller's txs.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/dagpu.h"
#include "runtime.hpp"
#include "square_plan.hpp"
#include "square_write.hpp"

namespace {

// the parse and layout arithmetic: square_plan.hpp, shared with the device planner
using namespace dagpu;

constexpr size_t kShare = 512, kNs = 29, kNsId = 28;
constexpr size_t kFirstCompact = 474, kContCompact = 478;  // content bytes

struct SquareError {
  std::string msg;
};

// ---- namespaces (pkg/namespace/consts.go) ----------------------------------
struct Ns {
  uint8_t b[kNs];
};
Ns primary_reserved(uint8_t last) {
  Ns n{};
  n.b[kNs - 1] = last;
  return n;
}
Ns secondary_reserved(uint8_t last) {
  Ns n;
  memset(n.b, 0xFF, kNs);
  n.b[kNs - 1] = last;
  return n;
}
const Ns kTxNs = primary_reserved(0x01);
const Ns kPfbNs = primary_reserved(0x04);
const Ns kReservedPaddingNs = primary_reserved(0xFF);
const Ns kTailPaddingNs = secondary_reserved(0xFE);

// namespace.From: version 0 or 255; a version-0 ID starts with 18 zero bytes
void validate_namespace(const uint8_t* ns) {
  const int fault = namespace_fault(ns);
  if (fault == 1) throw SquareError{"unsupported namespace version " + std::to_string(ns[0])};
  if (fault == 2)
    throw SquareError{"unsupported namespace id with version 0. ID must start with 18 leading zeros"};
}

void append_uvarint(std::vector<uint8_t>& o, uint64_t v) {
  uint8_t b[10];
  o.insert(o.end(), b, b + put_uvarint(b, v));
}

struct Span {
  const uint8_t* p = nullptr;
  size_t n = 0;
};

struct BlobRef {
  Span ns_id, data;
  uint32_t share_version = 0, ns_version = 0;
};

// blob.UnmarshalBlobTx (sp_unmarshal_blob_tx): is a blob tx iff it decodes,
// type_id == "BLOB", it carries blobs and every namespace ID is 28 bytes
bool unmarshal_blob_tx(Span buf, Span& inner, std::vector<BlobRef>& blobs, std::vector<SpBlobFields>& f) {
  blobs.clear();
  inner = {};
  // one pass in fill mode into the caller's scratch, which only grows: a blob
  // of a blob tx carries a 28-byte namespace ID, so it has 32 bytes or more
  if (f.size() < buf.n / 32 + 1) f.resize(buf.n / 32 + 1);
  const SpTxInfo info =
      sp_unmarshal_blob_tx(buf.p, (uint32_t)buf.n, 0, f.data(), (uint32_t)f.size(), sizeof(SpBlobFields));
  if (!info.is_blob_tx) return false;
  inner = {buf.p + info.inner_off, info.inner_len};
  for (uint32_t j = 0; j < info.nblob; j++) {
    const SpBlobFields& b = f[j];
    BlobRef r;
    r.ns_id = {buf.p + b.ns_off, b.ns_len};
    r.data = {buf.p + b.data_off, b.data_len};
    r.share_version = b.share_version;
    r.ns_version = b.ns_version;
    blobs.push_back(r);
  }
  return true;
}

// tmproto.IndexWrapper{tx = 1, share_indexes = 2 (packed), type_id = 3 "INDX"}
void marshal_index_wrapper(Span tx, const std::vector<uint32_t>& idx, std::vector<uint8_t>& o) {
  o.clear();
  if (tx.n) {
    o.push_back(0x0a);
    append_uvarint(o, tx.n);
    o.insert(o.end(), tx.p, tx.p + tx.n);
  }
  if (!idx.empty()) {
    size_t packed = 0;
    for (uint32_t x : idx) packed += uvarint_len(x);
    o.push_back(0x12);
    append_uvarint(o, packed);
    for (uint32_t x : idx) append_uvarint(o, x);
  }
  o.push_back(0x1a);
  o.push_back(4);
  o.insert(o.end(), {'I', 'N', 'D', 'X'});
}
void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24);
  p[1] = (uint8_t)(v >> 16);
  p[2] = (uint8_t)(v >> 8);
  p[3] = (uint8_t)v;
}
uint32_t get_be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

// namespace padding share: ns | info(version, start) | sequence len 0 | zeros
void padding_share(uint8_t* out, const uint8_t* ns, uint8_t version) {
  memcpy(out, ns, kNs);
  out[kNs] = (uint8_t)((version << 1) | 1);
  memset(out + kNs + 1, 0, kShare - kNs - 1);
}

// shares.CompactShareCounter (counter.go): compact shares a run of delimited units needs
struct CompactCounter {
  uint64_t last_shares = 0, last_rem = 0, shares = 0, rem = 0;
  int64_t add(uint64_t len) {
    uint64_t d = len + uvarint_len(len);
    last_rem = rem;
    last_shares = shares;
    if (shares == 0) {
      if (d >= kFirstCompact - rem) {
        d -= kFirstCompact - rem;
        shares++;
        rem = 0;
      } else {
        rem += d;
        d = 0;
      }
    }
    if (d >= kContCompact - rem) {
      d -= kContCompact - rem;
      shares++;
      rem = 0;
    } else {
      rem += d;
      d = 0;
    }
    if (d > 0) {
      shares += d / kContCompact;
      rem = d % kContCompact;
    }
    int64_t diff = (int64_t)shares - (int64_t)last_shares;
    if (last_rem == 0 && rem > 0) diff++;
    else if (last_rem > 0 && rem == 0) diff--;
    return diff;
  }
  void revert() {
    shares = last_shares;
    rem = last_rem;
  }
  uint64_t size() const { return rem == 0 ? shares : shares + 1; }
};

// shares.CompactShareSplitter: length-delimited units into compact shares
// (ns | info | [sequence len] | reserved = offset of the first unit starting
// in the share | data), written into an internal buffer.
class CompactWriter {
 public:
  explicit CompactWriter(const Ns& ns) : ns_(ns) { start(true); }
  void write_tx(Span tx) {
    uint8_t delim[10];
    const size_t dl = put_uvarint(delim, tx.n);
    // maybe_write_reserved_bytes: the first unit that starts in this share
    if (get_be32(cur_ + reserved_at()) == 0) put_be32(cur_ + reserved_at(), (uint32_t)len_);
    add(delim, dl);
    add(tx.p, tx.n);
    if (len_ == kShare) stack();
  }
  size_t count() const { return shares_.size() / kShare + (empty_share() ? 0 : 1); }
  // Export: zero-pads the last share and writes the sequence length
  void export_to(uint8_t* out) {
    if (shares_.empty() && empty_share()) return;
    size_t padding = 0;
    if (!empty_share()) {
      padding = kShare - len_;
      memset(cur_ + len_, 0, padding);
      len_ = kShare;
      stack();
    }
    const size_t n = shares_.size() / kShare;
    const size_t seq = kFirstCompact + (n - 1) * kContCompact - padding;
    put_be32(shares_.data() + kNs + 1, (uint32_t)seq);
    memcpy(out, shares_.data(), shares_.size());
  }

 private:
  Ns ns_;
  std::vector<uint8_t> shares_;
  uint8_t cur_[kShare];
  size_t len_ = 0;
  bool first_ = true;
  size_t reserved_at() const { return kNs + 1 + (first_ ? 4 : 0); }
  bool empty_share() const { return len_ == reserved_at() + 4; }
  void start(bool first) {
    first_ = first;
    memcpy(cur_, ns_.b, kNs);
    cur_[kNs] = first ? 1 : 0;  // share version 0
    len_ = kNs + 1;
    if (first) {
      memset(cur_ + len_, 0, 4);
      len_ += 4;
    }
    memset(cur_ + len_, 0, 4);
    len_ += 4;
  }
  void stack() {
    shares_.insert(shares_.end(), cur_, cur_ + kShare);
    start(false);
  }
  void add(const uint8_t* p, size_t n) {
    while (n) {
      if (len_ == kShare) stack();
      const size_t t = std::min(n, kShare - len_);
      memcpy(cur_ + len_, p, t);
      len_ += t;
      p += t;
      n -= t;
    }
  }
};

struct Element {
  BlobRef blob;
  size_t pfb_index, blob_index;
  uint64_t num_shares, max_padding;
  uint8_t ns[kNs];
};

struct PfbRec {
  Span tx;
  std::vector<uint32_t> share_indexes;
};

// pkg/square Builder
class SquareBuilder {
 public:
  SquareBuilder(uint64_t max_square_size, uint64_t threshold) : threshold_(threshold) {
    if (max_square_size == 0) throw SquareError{"max square size must be strictly positive"};
    if (max_square_size & (max_square_size - 1)) throw SquareError{"max square size must be a power of two"};
    max_capacity_ = max_square_size * max_square_size;
  }
  bool append_tx(Span tx) {
    const int64_t diff = tx_counter_.add(tx.n);
    if (fits(diff)) {
      txs_.push_back(tx);
      current_ += diff;
      return true;
    }
    tx_counter_.revert();
    return false;
  }
  bool append_blob_tx(Span inner, const std::vector<BlobRef>& blobs) {
    // worst case: every share index is SquareSizeUpperBound^2
    const size_t iw = index_wrapper_size(inner.n, blobs.size(), 128u * 128u);
    const int64_t pfb_diff = pfb_counter_.add(iw);
    int64_t max_blob = 0;
    std::vector<Element> el;
    for (size_t i = 0; i < blobs.size(); i++) {
      Element e{};
      e.blob = blobs[i];
      e.pfb_index = pfbs_.size();
      e.blob_index = i;
      e.num_shares = sparse_shares_needed(blobs[i].data.n);
      e.max_padding = subtree_width_u(e.num_shares, threshold_) - 1;
      e.ns[0] = (uint8_t)blobs[i].ns_version;
      memcpy(e.ns + 1, blobs[i].ns_id.p, kNsId);
      max_blob += (int64_t)(e.num_shares + e.max_padding);
      el.push_back(e);
    }
    if (fits(pfb_diff + max_blob)) {
      blobs_.insert(blobs_.end(), el.begin(), el.end());
      pfbs_.push_back({inner, std::vector<uint32_t>(blobs.size(), 128u * 128u)});
      current_ += pfb_diff + max_blob;
      return true;
    }
    pfb_counter_.revert();
    return false;
  }
  bool empty() const { return tx_counter_.size() == 0 && pfb_counter_.size() == 0; }
  // square size of the export (1 for the empty square)
  uint64_t square_size() const { return empty() ? 1 : blob_min_square_size((uint64_t)current_); }

  // The layout pass of Export + WriteSquare: where every run of shares starts,
  // with every check the reference makes while exporting, in its order.  Sorts
  // the blobs and fills in the PFBs' share indexes; writes no share.
  struct Layout {
    uint64_t ss = 1, total = 1;
    uint64_t tx_len = 0, pfb_len = 0;  // bytes of the two delimited unit streams
    uint64_t pfb_start = 0, padding_start = 0, non_reserved_start = 0, end_of_last_blob = 0;
    std::vector<uint64_t> start;  // first share of each blob, in blobs_ order
  };
  Layout layout() {
    Layout l;
    l.ss = square_size();
    l.total = l.ss * l.ss;
    if (empty()) return l;
    std::stable_sort(blobs_.begin(), blobs_.end(),
                     [](const Element& a, const Element& b) { return memcmp(a.ns, b.ns, kNs) < 0; });
    for (const Span& t : txs_) l.tx_len += uvarint_len(t.n) + t.n;
    uint64_t non_reserved_start = tx_counter_.size() + pfb_counter_.size();
    uint64_t cursor = non_reserved_start, end_of_last = non_reserved_start;
    l.start.resize(blobs_.size());
    for (size_t i = 0; i < blobs_.size(); i++) {
      Element& e = blobs_[i];
      const uint64_t wdt = subtree_width_u(e.num_shares, threshold_);
      cursor = next_share_index(cursor, wdt);
      if (i == 0) non_reserved_start = cursor;
      const uint64_t padding = cursor - end_of_last;
      if (padding > e.max_padding)
        throw SquareError{"blob has " + std::to_string(padding) + " padding shares, but " +
                          std::to_string(e.max_padding) + " was the max possible"};
      pfbs_[e.pfb_index].share_indexes[e.blob_index] = (uint32_t)cursor;
      l.start[i] = cursor;
      // the checks SparseShareSplitter makes while writing, in its order:
      // padding in the previous blob's namespace, then Blob.ValidateBasic
      if (i > 0 && padding > 0) validate_namespace(blobs_[i - 1].ns);
      if (e.blob.share_version > 255) throw SquareError{"share version can not be greater than MaxShareVersion"};
      if (e.blob.ns_version > 255)
        throw SquareError{"namespace version can not be greater than MaxNamespaceVersion"};
      if (e.blob.data.n == 0) throw SquareError{"blob data can not be empty"};
      if (e.blob.share_version != 0)
        throw SquareError{"unsupported share version: " + std::to_string(e.blob.share_version)};
      cursor += e.num_shares;
      end_of_last = cursor;
    }
    for (const PfbRec& p : pfbs_) {
      const size_t iw = index_wrapper_size(p.tx.n, p.share_indexes.data(), p.share_indexes.size());
      l.pfb_len += uvarint_len(iw) + iw;
    }
    const uint64_t pfb_count = compact_shares_needed(l.pfb_len);
    if (pfb_counter_.size() < pfb_count)
      throw SquareError{"pfbCounter.Size() < pfbTxWriter.Count(): " + std::to_string(pfb_counter_.size()) +
                        " < " + std::to_string(pfb_count)};
    // WriteSquare
    l.pfb_start = compact_shares_needed(l.tx_len);
    l.padding_start = l.pfb_start + pfb_count;
    if (non_reserved_start < l.padding_start)
      throw SquareError{"nonReservedStart " + std::to_string(non_reserved_start) +
                        " is too small to fit all PFBs and txs"};
    uint64_t blob_count = 0;
    for (size_t i = 0; i < blobs_.size(); i++) {
      blob_count += blobs_[i].num_shares;
      if (i > 0) blob_count += l.start[i] - (l.start[i - 1] + blobs_[i - 1].num_shares);
    }
    l.non_reserved_start = non_reserved_start;
    l.end_of_last_blob = non_reserved_start + blob_count;
    if (l.total < l.end_of_last_blob)
      throw SquareError{"square size " + std::to_string(l.total) + " is too small to fit all blobs"};
    if (blobs_.empty() && non_reserved_start != l.padding_start)
      throw SquareError{"square has unwritten shares"};
    return l;
  }

  // Export + WriteSquare into out (square_size()^2 shares)
  void export_to(uint8_t* out) {
    const Layout l = layout();
    if (empty()) {
      padding_share(out, kTailPaddingNs.b, 0);
      return;
    }
    CompactWriter txw(kTxNs);
    for (const Span& t : txs_) txw.write_tx(t);
    CompactWriter pfbw(kPfbNs);
    std::vector<uint8_t> iw;
    for (const PfbRec& p : pfbs_) {
      marshal_index_wrapper(p.tx, p.share_indexes, iw);
      pfbw.write_tx({iw.data(), iw.size()});
    }
    txw.export_to(out);
    pfbw.export_to(out + l.pfb_start * kShare);
    if (!blobs_.empty()) {
      for (uint64_t s = l.padding_start; s < l.non_reserved_start; s++)
        padding_share(out + s * kShare, kReservedPaddingNs.b, 0);
      uint8_t* o = out + l.non_reserved_start * kShare;
      for (size_t i = 0; i < blobs_.size(); i++) {
        const Element& e = blobs_[i];
        if (i > 0) {  // namespace padding in the previous blob's namespace
          const uint64_t pad = l.start[i] - (l.start[i - 1] + blobs_[i - 1].num_shares);
          for (uint64_t p = 0; p < pad; p++, o += kShare) padding_share(o, blobs_[i - 1].ns, 0);
        }
        o = write_blob(o, e);
      }
    }
    for (uint64_t s = l.end_of_last_blob; s < l.total; s++) padding_share(out + s * kShare, kTailPaddingNs.b, 0);
  }

  // The same square as a plan (square_write.hpp): the layout's tables, with
  // every source reference an offset from `base`, the caller's packed txs.
  // Copies no payload byte: only varint delimiters and IndexWrapper heads and
  // tails go into the literal pool.
  void plan_to(std::vector<uint8_t>& plan, const uint8_t* base, uint32_t src_bytes) {
    using namespace dagpu;
    const Layout l = layout();
    struct Seq {
      std::vector<uint32_t> seg, unit;
      uint32_t pos = 0;
      bool last_lit = false;
    } seq[2];
    std::vector<uint8_t> lit;
    auto add_lit = [&](Seq& q, const uint8_t* p, size_t n) {
      if (!n) return;
      if (!q.last_lit) {  // literals written back to back are one segment
        q.seg.push_back(q.pos);
        q.seg.push_back(kSqLitFlag | (uint32_t)lit.size());
      }
      lit.insert(lit.end(), p, p + n);
      q.pos += (uint32_t)n;
      q.last_lit = true;
    };
    auto add_src = [&](Seq& q, Span s) {
      if (!s.n) return;
      q.seg.push_back(q.pos);
      q.seg.push_back((uint32_t)(s.p - base));
      q.pos += (uint32_t)s.n;
      q.last_lit = false;
    };
    uint8_t tmp[32];
    if (!empty()) {
      seq[0].seg.reserve(4 * txs_.size() + 2);
      seq[0].unit.reserve(txs_.size());
      for (const Span& t : txs_) {
        seq[0].unit.push_back(seq[0].pos);
        add_lit(seq[0], tmp, put_uvarint(tmp, t.n));
        add_src(seq[0], t);
      }
      seq[1].seg.reserve(4 * pfbs_.size() + 2);
      seq[1].unit.reserve(pfbs_.size());
      std::vector<uint8_t> tail;
      for (const PfbRec& p : pfbs_) {
        seq[1].unit.push_back(seq[1].pos);
        size_t n = put_uvarint(tmp, index_wrapper_size(p.tx.n, p.share_indexes.data(), p.share_indexes.size()));
        if (p.tx.n) {  // marshal_index_wrapper's bytes around the inner tx
          tmp[n++] = 0x0a;
          n += put_uvarint(tmp + n, p.tx.n);
        }
        add_lit(seq[1], tmp, n);
        add_src(seq[1], p.tx);
        marshal_index_wrapper({}, p.share_indexes, tail);
        add_lit(seq[1], tail.data(), tail.size());
      }
    }
    for (Seq& q : seq) {
      q.seg.push_back(q.pos);
      q.seg.push_back(0);
    }
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    SqHdr h{};
    h.magic = kSqMagic;
    h.version = kSqVersion;
    h.k = (uint32_t)l.ss;
    h.n_tx = (uint32_t)l.pfb_start;
    h.pad_start = (uint32_t)l.padding_start;
    h.blob_start = (uint32_t)l.non_reserved_start;
    h.blob_end = (uint32_t)l.end_of_last_blob;
    h.nblob = (uint32_t)blobs_.size();
    h.src_bytes = src_bytes;
    size_t at = sizeof(SqHdr);
    for (int q = 0; q < 2; q++) {
      h.seq_len[q] = seq[q].pos;
      h.nseg[q] = (uint32_t)(seq[q].seg.size() / 2 - 1);
      h.seg_off[q] = (uint32_t)at;
      at = up16(at + seq[q].seg.size() * 4);
      h.nunit[q] = (uint32_t)seq[q].unit.size();
      h.unit_off[q] = (uint32_t)at;
      at = up16(at + seq[q].unit.size() * 4);
    }
    h.blob_off = (uint32_t)at;
    at = up16(at + blobs_.size() * kSqBlobWords * 4);
    h.lit_off = (uint32_t)at;
    h.lit_bytes = (uint32_t)lit.size();
    at = up16(at + lit.size());
    h.plan_bytes = (uint32_t)at;
    plan.assign(at, 0);
    for (int q = 0; q < 2; q++) {
      if (!seq[q].seg.empty()) memcpy(plan.data() + h.seg_off[q], seq[q].seg.data(), seq[q].seg.size() * 4);
      if (!seq[q].unit.empty()) memcpy(plan.data() + h.unit_off[q], seq[q].unit.data(), seq[q].unit.size() * 4);
    }
    for (size_t i = 0; i < blobs_.size(); i++) {
      const Element& e = blobs_[i];
      uint8_t* r = plan.data() + h.blob_off + i * kSqBlobWords * 4;
      memcpy(r, e.ns, kNs);
      const uint32_t w[4] = {(uint32_t)l.start[i], (uint32_t)e.num_shares, (uint32_t)(e.blob.data.p - base),
                             (uint32_t)e.blob.data.n};
      memcpy(r + 32, w, 16);
    }
    if (!lit.empty()) memcpy(plan.data() + h.lit_off, lit.data(), lit.size());
    memcpy(plan.data(), &h, sizeof h);
  }

 private:
  uint64_t threshold_, max_capacity_ = 0;
  int64_t current_ = 0;
  CompactCounter tx_counter_, pfb_counter_;
  std::vector<Span> txs_;
  std::vector<PfbRec> pfbs_;
  std::vector<Element> blobs_;

  bool fits(int64_t n) const { return current_ + n <= (int64_t)max_capacity_; }

  // SparseShareSplitter.Write: first share ns | info | sequence len | data,
  // continuation shares ns | info | data, the last zero-padded
  static uint8_t* write_blob(uint8_t* o, const Element& e) {
    const uint8_t* p = e.blob.data.p;
    size_t n = e.blob.data.n;
    bool first = true;
    while (true) {
      memcpy(o, e.ns, kNs);
      o[kNs] = first ? 1 : 0;
      size_t at = kNs + 1;
      if (first) {
        put_be32(o + at, (uint32_t)e.blob.data.n);
        at += 4;
      }
      const size_t t = std::min(n, kShare - at);
      memcpy(o + at, p, t);
      memset(o + at + t, 0, kShare - at - t);
      o += kShare;
      p += t;
      n -= t;
      first = false;
      if (n == 0) return o;
    }
  }
};

std::vector<Span> split_txs(const uint8_t* txs, const uint64_t* lens, size_t ntx) {
  std::vector<Span> v(ntx);
  size_t off = 0;
  for (size_t i = 0; i < ntx; i++) {
    // the parser of square_plan.hpp walks a tx with 32-bit offsets
    if (lens[i] > 0xFFFFFFFFull) throw SquareError{"tx at index " + std::to_string(i) + " has 4 GiB or more"};
    v[i] = {txs + off, (size_t)lens[i]};
    off += (size_t)lens[i];
  }
  return v;
}

// the loop of square.Construct (every tx must fit, normal txs first) or of
// square.Build (what does not fit is skipped, kept[i] = 0)
void append_all(SquareBuilder& b, const std::vector<Span>& v, bool build, uint8_t* kept) {
  std::vector<BlobRef> blobs;
  std::vector<SpBlobFields> scratch;
  bool seen_blob = false;
  for (size_t i = 0; i < v.size(); i++) {
    Span inner;
    if (build) {
      const bool ok = unmarshal_blob_tx(v[i], inner, blobs, scratch) ? b.append_blob_tx(inner, blobs) : b.append_tx(v[i]);
      if (kept) kept[i] = ok ? 1 : 0;
    } else if (unmarshal_blob_tx(v[i], inner, blobs, scratch)) {
      seen_blob = true;
      if (!b.append_blob_tx(inner, blobs))
        throw SquareError{"not enough space to append blob tx at index " + std::to_string(i)};
    } else {
      if (seen_blob)
        throw SquareError{"normal tx at index " + std::to_string(i) + " can not be appended after blob tx"};
      if (!b.append_tx(v[i])) throw SquareError{"not enough space to append tx at index " + std::to_string(i)};
    }
  }
}

int finish(dagpu_ctx* ctx, SquareBuilder& b, uint8_t* ods_out, size_t ods_cap, uint32_t* square_size) {
  const uint64_t k = b.square_size();
  if (square_size) *square_size = (uint32_t)k;
  const size_t need = (size_t)(k * k) * kShare;
  if (!ods_out || ods_cap < need)
    return set_err(ctx, DAGPU_ERR_ARG, "ods buffer too small: need " + std::to_string(need) + " bytes");
  b.export_to(ods_out);
  return DAGPU_OK;
}

int construct_or_build(dagpu_ctx* ctx, const uint8_t* txs, const uint64_t* tx_lens, size_t ntx,
                       uint32_t max_square_size, uint32_t subtree_root_threshold, uint8_t* ods_out, size_t ods_cap,
                       uint32_t* square_size, bool build, uint8_t* kept) {
  if (ntx && (!txs || !tx_lens)) return set_err(ctx, DAGPU_ERR_ARG, "txs and tx_lens are required when ntx > 0");
  if (subtree_root_threshold == 0) return set_err(ctx, DAGPU_ERR_ARG, "subtree_root_threshold must be > 0");
  try {
    SquareBuilder b(max_square_size, subtree_root_threshold);
    append_all(b, split_txs(txs, tx_lens, ntx), build, kept);
    return finish(ctx, b, ods_out, ods_cap, square_size);
  } catch (const SquareError& e) {
    return set_err(ctx, DAGPU_ERR_SQUARE, e.msg);
  } catch (const std::bad_alloc&) {
    return set_err(ctx, DAGPU_ERR_SQUARE, "out of host memory");
  }
}

int plan_fail(const std::string& msg) { return set_err(nullptr, DAGPU_ERR_ARG, "square plan: " + msg); }

}  // namespace

extern "C" {

int dagpu_square_construct(dagpu_ctx* ctx, const uint8_t* txs, const uint64_t* tx_lens, size_t ntx,
                           uint32_t max_square_size, uint32_t subtree_root_threshold, uint8_t* ods_out,
                           size_t ods_cap, uint32_t* square_size) {
  return construct_or_build(ctx, txs, tx_lens, ntx, max_square_size, subtree_root_threshold, ods_out, ods_cap,
                            square_size, false, nullptr);
}

int dagpu_square_build(dagpu_ctx* ctx, const uint8_t* txs, const uint64_t* tx_lens, size_t ntx,
                       uint32_t max_square_size, uint32_t subtree_root_threshold, uint8_t* ods_out,
                       size_t ods_cap, uint32_t* square_size, uint8_t* kept) {
  return construct_or_build(ctx, txs, tx_lens, ntx, max_square_size, subtree_root_threshold, ods_out, ods_cap,
                            square_size, true, kept);
}

int dagpu_square_plan(dagpu_ctx* ctx, const uint8_t* txs, const uint64_t* tx_lens, size_t ntx,
                      uint32_t max_square_size, uint32_t subtree_root_threshold, uint8_t* kept, uint8_t* plan_out,
                      size_t plan_cap, size_t* plan_bytes, uint32_t* square_size) {
  if (ntx && (!txs || !tx_lens)) return set_err(ctx, DAGPU_ERR_ARG, "txs and tx_lens are required when ntx > 0");
  if (subtree_root_threshold == 0) return set_err(ctx, DAGPU_ERR_ARG, "subtree_root_threshold must be > 0");
  try {
    SquareBuilder b(max_square_size, subtree_root_threshold);
    const std::vector<Span> v = split_txs(txs, tx_lens, ntx);
    if (ntx && (uint64_t)(v.back().p + v.back().n - txs) >= dagpu::kSqLitFlag)
      return set_err(ctx, DAGPU_ERR_UNSUPPORTED, "a square plan addresses at most 2 GiB of txs");
    append_all(b, v, kept != nullptr, kept);
    const uint64_t k = b.square_size();
    if (square_size) *square_size = (uint32_t)k;
    if (k > dagpu::kSqMaxWidth)
      return set_err(ctx, DAGPU_ERR_UNSUPPORTED,
                     "a square plan is at most " + std::to_string(dagpu::kSqMaxWidth) + " shares wide");
    std::vector<uint8_t> plan;
    b.plan_to(plan, txs, ntx ? (uint32_t)(v.back().p + v.back().n - txs) : 0);
    if (plan_bytes) *plan_bytes = plan.size();
    if (!plan_out || plan_cap < plan.size())
      return set_err(ctx, DAGPU_ERR_ARG, "plan buffer too small: need " + std::to_string(plan.size()) + " bytes");
    memcpy(plan_out, plan.data(), plan.size());
    return DAGPU_OK;
  } catch (const SquareError& e) {
    return set_err(ctx, DAGPU_ERR_SQUARE, e.msg);
  } catch (const std::bad_alloc&) {
    return set_err(ctx, DAGPU_ERR_SQUARE, "out of host memory");
  }
}

int dagpu_square_plan_check(const uint8_t* plan, size_t plan_bytes, size_t src_bytes) {
  using namespace dagpu;
  if (!plan || ((uintptr_t)plan & 3)) return plan_fail("the plan must be 4-byte aligned");
  if (plan_bytes < sizeof(SqHdr)) return plan_fail("shorter than its header");
  SqHdr h;
  memcpy(&h, plan, sizeof h);
  if (h.magic != kSqMagic || h.version != kSqVersion) return plan_fail("not a version-1 plan");
  if (h.plan_bytes != plan_bytes || plan_bytes >= kSqLitFlag)
    return plan_fail("size " + std::to_string(plan_bytes) + " differs from the header's " +
                     std::to_string(h.plan_bytes));
  if (h.k == 0 || (h.k & (h.k - 1)) || h.k > kSqMaxWidth) return plan_fail("bad width " + std::to_string(h.k));
  // a table of `bytes` bytes at `off`, inside the plan and behind the header
  auto inside = [&](uint32_t off, uint64_t bytes) {
    return (off & 3) == 0 && off >= sizeof(SqHdr) && off <= plan_bytes && bytes <= plan_bytes - off;
  };
  if (src_bytes < h.src_bytes)
    return plan_fail("made for " + std::to_string(h.src_bytes) + " bytes of txs, given " + std::to_string(src_bytes));
  if (!inside(h.lit_off, h.lit_bytes)) return plan_fail("literal pool out of range");
  const uint32_t total = h.k * h.k;
  if (!(h.n_tx <= h.pad_start && h.pad_start <= h.blob_start && h.blob_start <= h.blob_end && h.blob_end <= total))
    return plan_fail("runs out of order");
  for (int q = 0; q < 2; q++) {
    const std::string name = q ? "PFB sequence: " : "tx sequence: ";
    const uint32_t shares = q ? h.pad_start - h.n_tx : h.n_tx;
    if (h.seq_len[q] > (uint64_t)total * kSqContCompact || sq_compact_shares(h.seq_len[q]) != shares)
      return plan_fail(name + "length does not fill its shares");
    if (h.nseg[q] > plan_bytes || h.nunit[q] > plan_bytes || !inside(h.seg_off[q], ((uint64_t)h.nseg[q] + 1) * 8) ||
        !inside(h.unit_off[q], (uint64_t)h.nunit[q] * 4))
      return plan_fail(name + "table out of range");
    if ((h.seq_len[q] == 0) != (h.nseg[q] == 0)) return plan_fail(name + "segments do not match the length");
    const uint32_t* sg = (const uint32_t*)(plan + h.seg_off[q]);
    if (sg[0] != 0 || sg[2 * h.nseg[q]] != h.seq_len[q]) return plan_fail(name + "segments do not span the stream");
    for (uint32_t i = 0; i < h.nseg[q]; i++) {
      if (sg[2 * i] >= sg[2 * i + 2]) return plan_fail(name + "segment positions not increasing");
      const uint64_t len = sg[2 * i + 2] - sg[2 * i], from = sg[2 * i + 1] & ~kSqLitFlag;
      if (from + len > (sg[2 * i + 1] & kSqLitFlag ? (uint64_t)h.lit_bytes : (uint64_t)src_bytes))
        return plan_fail(name + "segment " + std::to_string(i) + " reads past its source");
    }
    const uint32_t* u = (const uint32_t*)(plan + h.unit_off[q]);
    for (uint32_t i = 0; i < h.nunit[q]; i++)
      if (u[i] >= h.seq_len[q] || (i && u[i] <= u[i - 1])) return plan_fail(name + "unit starts not increasing");
  }
  if (h.nblob > plan_bytes || !inside(h.blob_off, (uint64_t)h.nblob * kSqBlobWords * 4))
    return plan_fail("blob table out of range");
  if (h.nblob == 0 && !(h.pad_start == h.blob_start && h.blob_start == h.blob_end))
    return plan_fail("padding runs without a blob");
  const uint32_t* b = (const uint32_t*)(plan + h.blob_off);
  uint32_t next = h.blob_start;
  for (uint32_t i = 0; i < h.nblob; i++, b += kSqBlobWords) {
    const uint32_t first = b[8], count = b[9], off = b[10], len = b[11];
    if (i == 0 ? first != next : first < next) return plan_fail("blob " + std::to_string(i) + " out of order");
    if (len == 0 || count != sq_sparse_shares(len) || count > h.blob_end - first || first > h.blob_end)
      return plan_fail("blob " + std::to_string(i) + " does not fill its shares");
    if ((uint64_t)off + len > src_bytes) return plan_fail("blob " + std::to_string(i) + " reads past the txs");
    if (b[7] >> 8) return plan_fail("blob " + std::to_string(i) + " namespace not zero padded");
    next = first + count;
  }
  if (h.nblob && next != h.blob_end) return plan_fail("blobs do not end at the tail padding");
  return DAGPU_OK;
}

int dagpu_square_plan_write_host(const uint8_t* plan, size_t plan_bytes, const uint8_t* txs, size_t src_bytes,
                                 uint8_t* ods_out, size_t row_pitch) {
  using namespace dagpu;
  const int rc = dagpu_square_plan_check(plan, plan_bytes, src_bytes);
  if (rc != DAGPU_OK) return rc;
  const uint32_t k = ((const SqHdr*)plan)->k;
  if (!ods_out || (src_bytes && !txs)) return plan_fail("txs and ods_out are required");
  if (row_pitch < (size_t)k * kShare) return plan_fail("row_pitch below k * 512");
  const uint8_t* lit = plan + ((const SqHdr*)plan)->lit_off;
  for (uint32_t s = 0; s < k * k; s++) {
    const SqShareDesc d = sq_share_desc(plan, s);
    uint8_t* o = ods_out + (size_t)(s / k) * row_pitch + (size_t)(s % k) * kShare;
    for (uint32_t i = 0; i < kShare / 8; i++) {
      const uint64_t w = sq_share_word(d, lit, txs, i);
      memcpy(o + 8 * i, &w, 8);
    }
  }
  return DAGPU_OK;
}

}  // extern "C"
