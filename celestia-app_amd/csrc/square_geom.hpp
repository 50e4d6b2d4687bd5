// square_geom.hpp -- how the kernels that read squares resident in HBM
// (square_read.hip, square_units.hip) address them: square i at squares +
// i * square_stride, rows row_pitch apart, the packed ODS batch or Q0 inside an
// EDS batch, as dagpu_square_write_device takes them, with its limits,
// alignment checks and messages.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "runtime.hpp"
#include "square_read.hpp"

namespace dagpu {

struct SqGeom {
  const uint8_t* squares;
  uint64_t square_stride, row_pitch;
  uint32_t log2k, total;  // total = k * k
};

constexpr size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

__device__ inline const uint8_t* share_at(const SqGeom& g, uint32_t sq, uint32_t s) {
  const uint32_t row = s >> g.log2k, col = s - (row << g.log2k);
  return g.squares + sq * g.square_stride + row * g.row_pitch + (uint64_t)col * kSqShare;
}

// bytes [0, 40) of a share: its address is a multiple of 16
__device__ inline SqrHead load_head(const uint8_t* share) {
  const uint4 a = ((const uint4*)share)[0], b = ((const uint4*)share)[1];
  const uint2 c = *(const uint2*)(share + 32);
  const uint64_t w[5] = {a.x | (uint64_t)a.y << 32, a.z | (uint64_t)a.w << 32, b.x | (uint64_t)b.y << 32,
                         b.z | (uint64_t)b.w << 32, c.x | (uint64_t)c.y << 32};
  return sqr_decode(w);
}

__device__ inline uint32_t wave_sum(uint32_t v) {
  for (uint32_t d = 32; d; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// the argument checks the scan, the read and the tx index share with
// dagpu_square_write_device
inline int check_geometry(dagpu_ctx* ctx, uint32_t k, size_t n, const void* d_squares, size_t square_stride,
                          size_t row_pitch, const void* d_workspace, SqGeom& g) {
  if (!is_pow2(k) || k > kSqMaxWidth) return set_err(ctx, DAGPU_ERR_ARG, "square width must be a power of two <= 1024");
  if (!d_squares) return set_err(ctx, DAGPU_ERR_ARG, "null argument");
  if (((uintptr_t)d_squares | square_stride | row_pitch | (uintptr_t)d_workspace) & 15)
    return set_err(ctx, DAGPU_ERR_ARG, "d_squares, square_stride, row_pitch and d_workspace must be multiples of 16");
  if (row_pitch < (size_t)k * kSS || (n > 1 && square_stride < (size_t)(k - 1) * row_pitch + (size_t)k * kSS))
    return set_err(ctx, DAGPU_ERR_ARG, "row_pitch below k * 512 or square_stride below one square");
  if ((uint64_t)n * k * k > ((uint64_t)1 << 32)) return set_err(ctx, DAGPU_ERR_ARG, "more than 2^32 shares in one call");
  if (n > 65535) return set_err(ctx, DAGPU_ERR_ARG, "more than 65535 squares in one call");
  uint32_t log2k = 0;
  while ((1u << log2k) < k) log2k++;
  g = {(const uint8_t*)d_squares, (uint64_t)square_stride, (uint64_t)row_pitch, log2k, k * k};
  return DAGPU_OK;
}

}  // namespace dagpu
