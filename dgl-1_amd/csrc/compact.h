// What the device graph builders share (induced_subgraph.hip, traversal.hip,
// neighbor_sample.hip, line_graph.hip, degree_buckets.hip and the item list of
// typed_block.hip).
// Each of them counts, scans the counts with rocPRIM, lets the caller read a
// few status words, and fills: the workspace carving, the scan, the argument
// checks and the wave-level and row-level device helpers of that scheme are
// here once. The item-row kernel and the checks are defined in compact.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include <cstdint>

#include "common.h"
#include "launch.h"
#include "timing.h"

namespace dglhip {

inline int64_t round256(int64_t v) { return (v + 255) & ~int64_t(255); }

// A workspace as a list of sections, each starting 256-byte aligned: take()
// gives the section's offset and moves on.
struct Carve {
  int64_t off = 0;
  int64_t take(int64_t bytes) {
    const int64_t at = off;
    off += round256(bytes);
    return at;
  }
};

// Temporary storage of an inclusive int64 sum scan (rocPRIM) over len values.
inline size_t scan_bytes_i64(int64_t len) {
  size_t bytes = 0;
  HIP_CALL(rocprim::inclusive_scan(nullptr, bytes, static_cast<const int64_t*>(nullptr),
                                   static_cast<int64_t*>(nullptr), size_t(len),
                                   rocprim::plus<int64_t>()));
  return bytes;
}

// out[i] = in[0] + ... + in[i] for i < n, with ws_bytes of temporary storage.
inline void scan_i64(void* ws, int64_t ws_bytes, const int64_t* in, int64_t* out, int64_t n,
                     hipStream_t stream) {
  size_t bytes = size_t(ws_bytes);
  HIP_CALL(rocprim::inclusive_scan(ws, bytes, in, out, size_t(n), rocprim::plus<int64_t>(),
                                   stream));
}

// item_row[j], j < bound, = the last i in [0, num_rows] with item_ptr[i] <= j:
// the row that item j belongs to (rows without items share their successor's
// start and are skipped by taking the last), num_rows for the items past the
// end. One launch.
void launch_item_rows(int64_t num_rows, int64_t bound, const int64_t* item_ptr,
                      int32_t* item_row, hipStream_t stream);

void check_workspace(int64_t workspace_bytes, int64_t needed);

// `why` is the caller's sentence: who reads what on the host.
void check_not_capturing(hipStream_t stream, const char* why);

// The lanes of the wave before `lane`, as a ballot mask.
__device__ __forceinline__ unsigned long long lanes_below(int lane) {
  return (1ull << lane) - 1ull;
}

// The wave's lanes with `hit`, added to *counter by lane 0 (a validation
// counter, never a position). Every lane calls it.
__device__ __forceinline__ void wave_count(bool hit, int64_t* counter) {
  const unsigned long long mask = __ballot(hit);
  if (mask != 0 && (threadIdx.x & 63) == 0)
    atomicAdd(reinterpret_cast<unsigned long long*>(counter),
              static_cast<unsigned long long>(__popcll(mask)));
}

// Sum over the wave (every lane calls it), added to *counter by lane 0. An
// integer sum: the same whatever the order of the adds.
__device__ __forceinline__ void wave_add(int64_t x, int64_t* counter) {
  long long v = x;
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0 && v != 0)
    atomicAdd(reinterpret_cast<unsigned long long*>(counter),
              static_cast<unsigned long long>(v));
}

// The sum of c over the wave, in every lane.
__device__ __forceinline__ int64_t wave_sum(int64_t c) {
  long long v = c;
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Slots [*beg, *end) of row v (v in [0, N)), clamped to the index arrays.
__device__ __forceinline__ void row_range(const int64_t* indptr, int64_t nnz, int64_t v,
                                          int64_t* beg, int64_t* end) {
  int64_t b = indptr[v], e = indptr[v + 1];
  b = b < 0 ? 0 : (b > nnz ? nnz : b);
  e = e < b ? b : (e > nnz ? nnz : e);
  *beg = b;
  *end = e;
}

// The last i in [lo, hi] with ptr[i] <= key (ptr[lo] <= key is given).
__device__ __forceinline__ int64_t last_le(const int64_t* ptr, int64_t key, int64_t lo,
                                           int64_t hi) {
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (ptr[mid] <= key) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Slots [*beg, *end) of chunk c (of at most K slots) of the row [rb, re);
// false when the row has no such chunk.
__device__ __forceinline__ bool item_slots(int64_t rb, int64_t re, int64_t c, int64_t K,
                                           int64_t* beg, int64_t* end) {
  const int64_t b = rb + c * K;
  if (b >= re) return false;
  *beg = b;
  *end = b + K < re ? b + K : re;
  return true;
}

}  // namespace dglhip
