// What a segment kernel needs to place its work from the offsets alone, on the
// device: the clamp that keeps an offset inside the rows, and the segment of a
// row. (segment_topk, segment_knn, segment_fps and segment_reduce carry their
// own copies; segment_radius.hip is the first unit to include this one.)
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dglhip {

__device__ __forceinline__ int64_t clampi(int64_t v, int64_t lo, int64_t hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

// the segment that contains `row`: the smallest s with offsets[s + 1] > row
// (B if there is none)
__device__ __forceinline__ int64_t segment_of(const int64_t* __restrict__ offsets, int64_t B,
                                              int64_t row) {
  int64_t lo = 0, hi = B;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (offsets[mid + 1] > row) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

}  // namespace dglhip
