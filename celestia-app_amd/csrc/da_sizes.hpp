// da_sizes.hpp -- share, node and codec sizes.  Host arithmetic only (no HIP):
// kernels.hpp includes it, and so do the workspace layouts
// (repair_layout.hpp) that tests/host/ compiles without a GPU.
#pragma once

namespace dagpu {

constexpr int kShareSize = 512;
constexpr int kNsSize = 29;
constexpr int kNodeSize = 90;  // minNs(29) | maxNs(29) | sha256(32)
constexpr int kDigest = 32;
// Widest square: (2k)^2 x 512 B of EDS = 128 GiB at k = 8192 fits the 288 GB of
// HBM, k = 16384 (512 GiB) does not.  GF(2^16) above k = 128; register-resident
// kernels at k = 256 / 512, LDS-slice kernels (rs_gf16_wide.hip) above.
constexpr int kMaxK = 8192;
// Widest codec vector (rsmt2d.Codec Encode / Decode, dagpu_encode / dagpu_decode):
// Leopard GF(2^16)'s whole field, k data + k parity = 65536 shards (klauspost
// leopardFF16 rejects more; rsmt2d LeoRSCodec.MaxChunks = 32768 * 32768).  A
// vector is k x shard bytes, so these widths fit one GPU even where the square
// of the same width does not; the wide kernels serve k = 16384 / 32768 with
// 2- / 1-symbol LDS slices (rs_gf16_wide.hip).
constexpr int kMaxCodecK = 32768;
// Widest split square (split.cpp, one oversized square over P GPUs): k = 16384,
// whose 512 GiB EDS one GPU cannot hold, over P >= kMinWideSplitParts ranks
// (P = 8: per rank a 64 GiB column slab, 32 GiB of row staging and send
// block, ~38 GiB of forest records -- under 288 GB; P = 4 would not fit).
constexpr int kMaxSplitK = 2 * kMaxK;
constexpr int kMinWideSplitParts = 8;

// Bytes of error-locator workspace per decoded vector.
// Error-locator workspace per vector: GF(2^8) 256 B; GF(2^16) the n = 2k uint16
// locators (4k B) and after them, at rs_err_tab_off(k), what the decoders'
// per-element multiplies need, built once per erasure pattern by the locator
// kernel (round 6) instead of in every decoder workgroup: at k = 256 / 512 the
// n x 80-B image of the product tables (exp(errLoc) for a present element,
// exp(-errLoc) for a missing one) that a half-lane decoder copies into LDS;
// at k >= 1024 the n x 32-B basis products (1 << b) * that factor, b < 16, from
// which a wide decoder workgroup builds an element's table without gathers.
constexpr long rs_err_tab_off(int k) { return 4L * k; }
constexpr long rs_err_elem_bytes(int k) { return k <= 1024 ? 80 : 32; }
constexpr long rs_err_bytes(int k) { return k <= 128 ? 256 : 4L * k + 2L * k * rs_err_elem_bytes(k); }

}  // namespace dagpu
