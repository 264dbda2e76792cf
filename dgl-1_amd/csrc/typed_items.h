// The chunked items of the typed-edge kernels (typed_block.hip,
// typed_linear.hip): a row (or relation) of deg slots is cut into
// max(1, ceil(deg / DGLHIP_TYPED_CHUNK)) items, each one chain from zero, and
// the partials of a row of several items are added in item order.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dgl_hip.h"

namespace dglhip {

constexpr int64_t kChunk = DGLHIP_TYPED_CHUNK;

// The slot range of item `it` of the chunked rows (item_ptr: a row's first
// item; a row of deg slots has max(1, ceil(deg / kChunk)) items) and where
// its chain goes: the row itself when the row is one item, else the item's
// partial row.
// Items past the last row's (item_row[it] >= num_rows: the caller sized the
// item list by its bound num_rows + nnz / kChunk, no host sync) do nothing.
__device__ __forceinline__ bool item_range(int64_t it, int64_t num_rows,
                                           const int64_t* __restrict__ ptr,
                                           const int64_t* __restrict__ item_ptr,
                                           const int32_t* __restrict__ item_row, int64_t* row,
                                           int64_t* beg, int64_t* end, bool* single) {
  const int64_t r = item_row[it];
  if (r >= num_rows) return false;
  const int64_t first = item_ptr[r], nit = item_ptr[r + 1] - first;
  const int64_t b = ptr[r] + (it - first) * kChunk;
  *row = r;
  *beg = b;
  *end = nit == 1 ? ptr[r + 1] : (b + kChunk < ptr[r + 1] ? b + kChunk : ptr[r + 1]);
  *single = nit == 1;
  return true;
}

// out[row] = ((p0 + p1) + p2) ... over the items of each row of several
// items, in item order (typed_block_combine_kernel in typed_block.hip; one
// timed launch). heavy_row NULL: every row, those of one item skipped.
void launch_typed_combine(int64_t num_heavy, int64_t F, const int32_t* heavy_row,
                          const int64_t* item_ptr, const float* partial, float* out,
                          const float* row_scale, hipStream_t stream);

}  // namespace dglhip
