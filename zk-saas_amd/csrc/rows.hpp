// Rows by pointer table: the copy between the separately allocated rows of a rank's k local callers (zk_party_*,
// engine_party.inc.hpp) and ONE staging block [items][k][row] that a rank call (zk_dist_*) can take.  Up to ROWS_MAX = 96
// rows per launch: three operands of 32 parties, or circom_h's three vectors in one launch.
//   - the pointer table travels BY VALUE in the kernel arguments (96 x 8 = 768 bytes): no table upload, no extra dependency
//   - blockIdx.y selects the row, so the row pointer is uniform per workgroup and is read with scalar loads
//   - the copy is 16-byte vector loads and stores, consecutive lanes at consecutive addresses; a grid-stride loop over the row
//     makes a one-element row and a row of 2^19 elements the same code
//   - one body, a direction flag: gather = rows -> block, scatter = block -> rows
// Rows and the block are 16-byte aligned and a row is a multiple of 16 bytes (every element type of the library is: 32-byte
// Fr, affine points of 64 .. 192 bytes); the launcher refuses anything else.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace zk {

constexpr int ROWS_MAX = 96;
struct RowTable {
  void* p[ROWS_MAX];
};
static_assert(sizeof(RowTable) == 768, "the table is the kernel's argument block");

template <bool SCATTER>
__device__ __forceinline__ void rows_copy_body(const RowTable& t, uint4* __restrict__ block, uint32_t row16) {
  const uint32_t row = blockIdx.y;                          // uniform: t.p[row] is a scalar load from the argument block
  uint4* ext = (uint4*)t.p[row];
  uint4* stg = block + (size_t)row * row16;
  const uint4* __restrict__ src = SCATTER ? stg : ext;
  uint4* __restrict__ dst = SCATTER ? ext : stg;
  const uint32_t step = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < row16; i += step) dst[i] = src[i];
}

// rows t.p[0 .. gridDim.y) of row16 16-byte words each -> block [gridDim.y][row16]
// (static: the header is included by one translation unit per curve)
static __global__ void __launch_bounds__(256) rows_gather_kernel(RowTable t, uint4* __restrict__ block, uint32_t row16) {
  rows_copy_body<false>(t, block, row16);
}
// block [gridDim.y][row16] -> rows t.p[0 .. gridDim.y)
static __global__ void __launch_bounds__(256) rows_scatter_kernel(RowTable t, uint4* __restrict__ block, uint32_t row16) {
  rows_copy_body<true>(t, block, row16);
}

// Launch shape: 256 threads; grid.y = rows; grid.x = what covers the row at one word per thread, capped so that the whole
// grid stays near 2048 workgroups (256 CUs x 8) and the rest is walked by the grid-stride loop.  A 2^20 d_fft at l = 2, k = 8:
// 8 rows of 2^20 words -> 256 x 8 workgroups, 16 words per thread.
inline hipError_t rows_launch(bool scatter, const RowTable& t, int rows, void* block, size_t row_bytes, hipStream_t st) {
  if (rows <= 0 || !row_bytes) return hipSuccess;
  if (rows > ROWS_MAX || (row_bytes & 15) || ((uintptr_t)block & 15) || (row_bytes >> 4) > 0x7fffffffull) return hipErrorInvalidValue;
  for (int i = 0; i < rows; i++)
    if (!t.p[i] || ((uintptr_t)t.p[i] & 15)) return hipErrorInvalidValue;
  const uint32_t row16 = (uint32_t)(row_bytes >> 4);
  uint32_t gx = (row16 + 255) / 256, cap = 2048u / (uint32_t)rows;
  if (cap < 1) cap = 1;
  if (gx > cap) gx = cap;
  if (scatter) rows_scatter_kernel<<<dim3(gx, (unsigned)rows), dim3(256), 0, st>>>(t, (uint4*)block, row16);
  else rows_gather_kernel<<<dim3(gx, (unsigned)rows), dim3(256), 0, st>>>(t, (uint4*)block, row16);
  return hipGetLastError();
}

}  // namespace zk
