// Long rows cut into pieces, shared by the kernels that walk a CSR row by row
// (edge_softmax.hip, and through attention_walk.h dot_attention.hip and
// gatv2_attention.hip). A row of more than `chunk` slots is cut where it
// crosses the multiples of the chunk: block g is slots
// [g chunk, (g + 1) chunk), and it meets at most two long rows, the one that
// holds its first slot (item 2 g) and one that starts inside it (item
// 2 g + 1). The geometry comes from the sizes alone: 2 G items for G blocks.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dglhip {

__device__ __forceinline__ int64_t clampi(int64_t v, int64_t lo, int64_t hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

// The row that holds `slot`: the smallest r with indptr[r + 1] > slot (R if
// none), found by the whole wave: every round its 64 lanes probe the range at
// even steps and a ballot keeps the step that holds the answer, so 2^18 rows
// take three dependent loads instead of eighteen. Every lane must call it.
__device__ __forceinline__ int64_t row_of(const int64_t* __restrict__ indptr, int64_t R,
                                          int64_t slot, int lane) {
  int64_t lo = 0, hi = R;  // the answer is in [lo, hi]
  while (lo < hi) {
    const int64_t step = (hi - lo + 63) >> 6;
    int64_t r = lo + (lane + 1) * step - 1;  // the last row of this lane's step
    if (r > hi - 1) r = hi - 1;
    const unsigned long long above = __ballot(indptr[r + 1] > slot);
    if (above == 0) return hi;
    const int j = __ffsll(above) - 1;
    const int64_t rj = lo + (j + 1) * step - 1;
    hi = rj > hi - 1 ? hi - 1 : rj;
    lo = lo + j * step;
  }
  return lo;
}

// The piece of a long row that item `item` of G blocks stands for: slots
// [k0, k1) of row r; `first` is the item of the row's first piece and `last`
// the block of its last one (the pieces after the first are the items 2 g of
// the blocks first / 2 < g <= last). False when the item has no piece. The
// same in every lane; every lane must call it.
__device__ __forceinline__ bool long_row_piece(const int64_t* __restrict__ indptr, int64_t R,
                                               int64_t nnz, int64_t G, int64_t chunk,
                                               int64_t item, int lane, int64_t& r, int64_t& k0,
                                               int64_t& k1, int64_t& first, int64_t& last) {
  const int64_t g = item >> 1;
  const bool inner = item & 1;
  const int64_t b0 = g * chunk;
  if (g >= G || b0 >= nnz) return false;
  const int64_t b1 = b0 + chunk < nnz ? b0 + chunk : nnz;
  r = row_of(indptr, R, inner ? b1 - 1 : b0, lane);
  if (r >= R) return false;
  const int64_t beg = clampi(indptr[r], 0, nnz);
  const int64_t end = clampi(indptr[r + 1], beg, nnz);
  if (end - beg <= chunk) return false;
  if (inner ? beg <= b0 : beg > b0) return false;
  k0 = beg > b0 ? beg : b0;
  k1 = end < b1 ? end : b1;
  const int64_t g0 = beg / chunk;
  first = 2 * g0 + (beg > g0 * chunk ? 1 : 0);
  last = (end - 1) / chunk;
  return k0 < k1;
}

}  // namespace dglhip
