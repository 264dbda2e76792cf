// Shared part of the g-SpMM kernels (sum / mean / max, every message and
// edge-feature layout) and their launch logic. Included by gspmm.hip (the
// C-ABI, which only declares the two dispatch_me overloads) and by
// gspmm_inst.hip, which is compiled once per (message, edge layout) pair
// (-DGSPMM_INST_MSG / -DGSPMM_INST_EM, see the Makefile) and instantiates
// them, so the kernel variants build in parallel translation units.
// Design notes: gspmm.hip header and DESIGN.md §4.1.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <mutex>
#include <vector>

#include "../../include/dgl_hip.h"
#include "common.h"
#include "launch.h"
#include "timing.h"

namespace dglhip {

// GAT attention dropout: keep(k, h) = hash(seed, k * H + h) >= threshold, a
// stateless counter hash shared by the fused forward (gat_fused.hip), the
// backward epilogues (gspmm.hip) and the host mask.
// lowbias32 (a 32-bit integer finaliser); two rounds over the 64-bit index
__host__ __device__ __forceinline__ uint32_t gat_mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

__host__ __device__ __forceinline__ bool gat_keep(uint64_t seed, int64_t idx, uint32_t thr) {
  const uint64_t i = static_cast<uint64_t>(idx);
  const uint32_t r = gat_mix32(gat_mix32(static_cast<uint32_t>(i) ^ static_cast<uint32_t>(seed)) ^
                               (static_cast<uint32_t>(i >> 32) + static_cast<uint32_t>(seed >> 32) +
                                0x9e3779b9u));
  return r >= thr;
}

// keep iff hash >= threshold: P(keep) = 1 - p
static inline uint32_t gat_drop_threshold(float p) {
  const double t = static_cast<double>(p) * 4294967296.0;
  return t >= 4294967295.0 ? 0xffffffffu : static_cast<uint32_t>(t);
}

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int VEC> struct Vec;
template <> struct Vec<1> {
  typedef float T;
  static __device__ __forceinline__ T zero() { return 0.0f; }
  static __device__ __forceinline__ T splat(float x) { return x; }
  static __device__ __forceinline__ T fma(T a, T b, T c) { return __builtin_fmaf(a, b, c); }
  static __device__ __forceinline__ T max(T a, T b) { return a > b ? a : b; }
};
template <> struct Vec<2> {
  typedef f32x2 T;
  static __device__ __forceinline__ T zero() { return T{0.0f, 0.0f}; }
  static __device__ __forceinline__ T splat(float x) { return T{x, x}; }
  static __device__ __forceinline__ T fma(T a, T b, T c) {
    return T{__builtin_fmaf(a.x, b.x, c.x), __builtin_fmaf(a.y, b.y, c.y)};
  }
};
template <> struct Vec<4> {
  typedef f32x4 T;
  static __device__ __forceinline__ T zero() { return T{0.0f, 0.0f, 0.0f, 0.0f}; }
  static __device__ __forceinline__ T splat(float x) { return T{x, x, x, x}; }
  static __device__ __forceinline__ T fma(T a, T b, T c) {
    return T{__builtin_fmaf(a.x, b.x, c.x), __builtin_fmaf(a.y, b.y, c.y),
             __builtin_fmaf(a.z, b.z, c.z), __builtin_fmaf(a.w, b.w, c.w)};
  }
};

template <int VEC>
__device__ __forceinline__ typename Vec<VEC>::T ldv(const float* p) {
  return *reinterpret_cast<const typename Vec<VEC>::T*>(p);
}
template <int VEC>
__device__ __forceinline__ void stv(float* p, typename Vec<VEC>::T v) {
  *reinterpret_cast<typename Vec<VEC>::T*>(p) = v;
}

// DGLHIP_MSG_COPY_U_BF16: copy_u over source rows held as bf16 bits. Each
// value widens exactly to fp32 (bits << 16) before it enters the fp32 chain,
// so results equal the fp32 kernel on the widened rows, bit for bit.
__host__ __device__ constexpr bool copies_u(int msg) {
  return msg == DGLHIP_MSG_COPY_U || msg == DGLHIP_MSG_COPY_U_BF16;
}

template <int VEC>
__device__ __forceinline__ typename Vec<VEC>::T gather_bf16(const float* ufeat, int32_t col,
                                                            int64_t F, int64_t f0);
template <>
__device__ __forceinline__ float gather_bf16<1>(const float* ufeat, int32_t col, int64_t F,
                                                int64_t f0) {
  const uint16_t b = reinterpret_cast<const uint16_t*>(ufeat)[int64_t(col) * F + f0];
  return __uint_as_float(uint32_t(b) << 16);
}
template <>
__device__ __forceinline__ f32x2 gather_bf16<2>(const float* ufeat, int32_t col, int64_t F,
                                                int64_t f0) {
  // two consecutive bf16 values, element f0 in the low half (little endian)
  const uint32_t w = *reinterpret_cast<const uint32_t*>(
      reinterpret_cast<const uint16_t*>(ufeat) + int64_t(col) * F + f0);
  return f32x2{__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u)};
}
template <>
__device__ __forceinline__ f32x4 gather_bf16<4>(const float* ufeat, int32_t col, int64_t F,
                                                int64_t f0) {
  typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
  const u32x2 w = *reinterpret_cast<const u32x2*>(
      reinterpret_cast<const uint16_t*>(ufeat) + int64_t(col) * F + f0);
  return f32x4{__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u),
               __uint_as_float(w.y << 16), __uint_as_float(w.y & 0xffff0000u)};
}

// Cache policy of the output stores (POL template parameter; copy_u + sum at
// VEC 2 x 64 lanes, see stream_output):
//  POL_DEFAULT : default policy everywhere.
//  POL_NT_OUT  : the output store non-temporal.
// (Non-temporal gathers, and gathers non-temporal for all but flagged "hot"
// source rows, were measured and removed: DESIGN.md, the r01 cache-policy study.)
enum { POL_DEFAULT = 0, POL_NT_OUT = 3 };

// BUF: the row is wave-uniform (a whole wave per row, the column id from the
// scalar slot stream): gather it through a buffer descriptor built from the
// row's address, so every gather in flight shares the lane's one 32-bit byte
// offset instead of holding a 64-bit address of its own (VGPRs -> waves per
// SIMD). Same loads, same values.
template <int VEC>
__device__ __forceinline__ typename Vec<VEC>::T gather_row_buf(const float* row, int64_t F,
                                                               int64_t f0) {
  typedef typename Vec<VEC>::T V;
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(row), 0, static_cast<int>(F * int64_t(sizeof(float))), 0x00020000);
  const uint32_t off = static_cast<uint32_t>(f0 * int64_t(sizeof(float)));
  if (VEC == 4) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
    return *reinterpret_cast<const V*>(&w);
  }
  if (VEC == 2) {
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    const u32x2 w = __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0);
    return *reinterpret_cast<const V*>(&w);
  }
  const unsigned int w = __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0);
  return *reinterpret_cast<const V*>(&w);
}

template <int VEC, bool BUF>
__device__ __forceinline__ typename Vec<VEC>::T gather_row(const float* __restrict__ ufeat,
                                                           int32_t col, int64_t F, int64_t f0) {
  if (BUF) return gather_row_buf<VEC>(ufeat + int64_t(col) * F, F, f0);
  return ldv<VEC>(ufeat + int64_t(col) * F + f0);
}

// Output rows: non-temporal under POL_NT_OUT. The policy is
// a template parameter, not a runtime flag: the compiler merges a branch
// between a plain and a non-temporal store into one plain store.
template <int VEC, int POL>
__device__ __forceinline__ void store_row(float* p, typename Vec<VEC>::T v) {
  if (POL == POL_DEFAULT) stv<VEC>(p, v);
  else __builtin_nontemporal_store(v, reinterpret_cast<typename Vec<VEC>::T*>(p));
}

// Edge-feature layouts (EM template parameter):
//  EM_FULL   : one value per edge and feature, efeat[e, f]
//  EM_SCALAR : one scalar per edge broadcast over the row, efeat[e]
//  EM_HEAD   : one scalar per edge and head, efeat[e, f / D] with D = F / elen
//              (GAT's (E, H, 1) attention against (N, H, D) features)
enum { EM_FULL = 0, EM_SCALAR = 1, EM_HEAD = 2 };

// Message for slot k as a vector of VEC features starting at feature f0.
//  COPY_U : u                     U_MUL_E: w * u (fused into the reducer)
//  COPY_E : e
// `eoff` is the edge-feature column of f0 (f0, 0 or f0 / D by EM).
template <int VEC, int MSG, int EM, bool BUF = false>
struct SlotLoad {
  typedef typename Vec<VEC>::T V;
  V u;
  V e;
  __device__ __forceinline__ void load(const float* __restrict__ ufeat,
                                       const float* __restrict__ efeat, int64_t ldu,
                                       int64_t F, int64_t f0, int64_t elen, int64_t eoff,
                                       int32_t src, int64_t edge) {
    // ldu: row stride of ufeat in elements (F, or a padded width)
    if (MSG == DGLHIP_MSG_COPY_U_BF16) u = gather_bf16<VEC>(ufeat, src, ldu, f0);
    else if (MSG != DGLHIP_MSG_COPY_E) u = gather_row<VEC, BUF>(ufeat, src, ldu, f0);
    if (!copies_u(MSG)) {
      if (EM == EM_FULL) e = ldv<VEC>(efeat + edge * F + f0);
      else e = Vec<VEC>::splat(efeat[edge * elen + eoff]);
    }
  }
};

// Sequential reduction of slots [beg, end) of one row for the VEC features at
// f0: the fma chain the reference's product runs (see the file header).
template <int VEC, int UNROLL, int MSG, int EM, bool USE_EID, bool BUF = false>
__device__ __forceinline__ typename Vec<VEC>::T reduce_range(
    typename Vec<VEC>::T acc, int64_t beg, int64_t end, int64_t ldu, int64_t F, int64_t f0,
    int64_t elen, int64_t eoff, const int32_t* __restrict__ indices,
    const int64_t* __restrict__ eid, const float* __restrict__ ufeat,
    const float* __restrict__ efeat) {
  int64_t k = beg;
  for (; k + UNROLL <= end; k += UNROLL) {
    SlotLoad<VEC, MSG, EM, BUF> s[UNROLL];
#pragma unroll
    for (int j = 0; j < UNROLL; ++j)
      s[j].load(ufeat, efeat, ldu, F, f0, elen, eoff, indices[k + j],
                copies_u(MSG) ? 0 : (USE_EID ? eid[k + j] : k + j));
#pragma unroll
    for (int j = 0; j < UNROLL; ++j) {
      if (copies_u(MSG)) acc += s[j].u;
      else if (MSG == DGLHIP_MSG_COPY_E) acc += s[j].e;
      else acc = Vec<VEC>::fma(s[j].e, s[j].u, acc);
    }
  }
  // the last rem < UNROLL slots as one predicated batch: all their gathers in
  // flight together (a slot-by-slot tail would serialise up to UNROLL - 1
  // load latencies per row, which dominates rows shorter than UNROLL)
  const int64_t rem = end - k;
  if (rem > 0) {
    SlotLoad<VEC, MSG, EM, BUF> s[UNROLL];
#pragma unroll
    for (int j = 0; j < UNROLL - 1; ++j)
      if (j < rem)
        s[j].load(ufeat, efeat, ldu, F, f0, elen, eoff, indices[k + j],
                  copies_u(MSG) ? 0 : (USE_EID ? eid[k + j] : k + j));
#pragma unroll
    for (int j = 0; j < UNROLL - 1; ++j) {
      if (j < rem) {
        if (copies_u(MSG)) acc += s[j].u;
        else if (MSG == DGLHIP_MSG_COPY_E) acc += s[j].e;
        else acc = Vec<VEC>::fma(s[j].e, s[j].u, acc);
      }
    }
  }
  return acc;
}

// Cache policy of the running output row of accumulating items (the
// blocked schedule's launches after the first read and rewrite each item's
// row: 30 % of the fabric bytes, streaming through the L2s that hold the
// gathered source block). RP:
//   0  plain load and store;
//   2  non-temporal load, store with sc1 (the line leaves the XCD's L2): the
//      accumulating launches (Reddit-shaped headline 3.83 -> 3.74 ms; the
//      source rows keep the L2s);
//   4  plain load, store with sc1: the first launch, which only writes its rows.
// Same values in every variant. (Non-temporal stores, 1, and system-scope
// loads, 3, lost the r04 A/B and were removed: DESIGN.md §4.1.)
template <int VEC, int RP>
__device__ __forceinline__ typename Vec<VEC>::T load_out(const float* row, int64_t f0) {
  typedef typename Vec<VEC>::T V;
  if (RP == 2) return __builtin_nontemporal_load(reinterpret_cast<const V*>(row + f0));
  return ldv<VEC>(row + f0);
}

template <int VEC, int RP>
__device__ __forceinline__ void store_out(float* row, int64_t f0, typename Vec<VEC>::T v) {
  if ((RP == 2 || RP == 4) && VEC == 2) {
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(row, 0, 0x7fffffff,
                                                                       0x00020000);
    __builtin_amdgcn_raw_buffer_store_b64(*reinterpret_cast<const u32x2*>(&v), r,
                                          static_cast<uint32_t>(f0 * int64_t(sizeof(float))),
                                          0, 16);
    return;
  }
  if ((RP == 2 || RP == 4) && VEC == 4) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(row, 0, 0x7fffffff,
                                                                       0x00020000);
    __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4*>(&v), r,
                                           static_cast<uint32_t>(f0 * int64_t(sizeof(float))),
                                           0, 16);
    return;
  }
  stv<VEC>(row + f0, v);
}

// Sum-reduce kernel (also MEAN). GROUP lanes per work item, VEC floats per
// lane. A work item is a whole row (CHUNKED = false: item i = row_order[i]),
// or a slot range [chunk_beg[i], chunk_end[i]) whose sum goes to out[i, :]
// (CHUNKED = true). With ACCUM the chain continues from the value already in
// out[i, :] (segment-by-segment evaluation of one sequential chain); with
// MEAN and ACCUM on whole rows the row's mean is added to the value in
// out[i, :] (out + mean: a sum of two terms, the same bits either way round).
template <int VEC, int GROUP, int UNROLL, int MSG, int EM, bool MEAN, bool CHUNKED,
          bool ACCUM, int POL = POL_DEFAULT, bool BUF = false, int RP = 0>
__global__ __launch_bounds__(256) void gspmm_sum_kernel(
    int64_t num_items, int64_t F, int64_t elen, int64_t ldu,
    const int64_t* __restrict__ indptr,
    const int32_t* __restrict__ indices, const int64_t* __restrict__ eid,
    const float* __restrict__ ufeat, const float* __restrict__ efeat,
    float* __restrict__ out, const int32_t* __restrict__ row_order,
    const int64_t* __restrict__ chunk_beg, const int64_t* __restrict__ chunk_end) {
  typedef typename Vec<VEC>::T V;
  constexpr int ITEMS_PER_WAVE = 64 / GROUP;
  const int lane = threadIdx.x & 63;
  // wave index is uniform; make that explicit so slot data goes through SGPRs
  const int64_t wave =
      block_linear() * (blockDim.x >> 6) +
      __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int64_t it = wave * ITEMS_PER_WAVE + (GROUP == 64 ? 0 : lane / GROUP);
  if (it >= num_items) return;
  const int gl = GROUP == 64 ? lane : (lane % GROUP);
  int64_t row, beg, end;
  if (CHUNKED) {
    // item it: slots [chunk_beg[it], chunk_end[it]) into row row_order[it]
    // (the blocked schedule's items), or into partial row it (heavy-row
    // chunks, row ranges); the three loads are independent
    row = row_order ? row_order[it] : it;
    if (GROUP == 64) row = __builtin_amdgcn_readfirstlane(static_cast<int>(row));
    beg = chunk_beg[it];
    end = chunk_end[it];
  } else {
    row = row_order ? row_order[it] : it;
    if (GROUP == 64) row = __builtin_amdgcn_readfirstlane(static_cast<int>(row));
    beg = indptr[row];
    end = indptr[row + 1];
  }
  for (int64_t f0 = int64_t(gl) * VEC; f0 < F; f0 += int64_t(GROUP) * VEC) {
    const int64_t eoff = EM == EM_HEAD ? f0 / (F / elen) : (EM == EM_FULL ? f0 : 0);
    constexpr bool ADD_MEAN = MEAN && ACCUM && !CHUNKED;
    V acc = (ACCUM && !ADD_MEAN) ? load_out<VEC, RP>(out + row * F, f0) : Vec<VEC>::zero();
    if (copies_u(MSG) || eid != nullptr)  // uniform branch
      acc = reduce_range<VEC, UNROLL, MSG, EM, true, BUF && GROUP == 64>(
          acc, beg, end, ldu, F, f0, elen, eoff, indices, eid, ufeat, efeat);
    else
      acc = reduce_range<VEC, UNROLL, MSG, EM, false>(acc, beg, end, ldu, F, f0, elen, eoff, indices,
                                                      eid, ufeat, efeat);
    if (!CHUNKED && MEAN && end - beg > 1)
      acc = acc / Vec<VEC>::splat(static_cast<float>(end - beg));
    if (ADD_MEAN) acc = ldv<VEC>(out + row * F + f0) + acc;
    if (RP) store_out<VEC, RP>(out + row * F, f0, acc);
    else store_row<VEC, POL>(out + row * F + f0, acc);
  }
}

// Two items per wave: the blocked schedule's items for copy_u over fp32 rows
// of 128 floats (DESIGN.md §4.1 "Two items per wave"). Wave w takes items 2w
// (lanes 0-31) and 2w + 1 (lanes 32-63), each lane 4 consecutive floats, so
// one gather instruction fetches two whole source rows (1 KiB) and a short
// item's round trips carry twice the payload. Both items' column ids come
// from the scalar slot stream; a lane picks its half's id and gathers at a
// 32-bit byte offset from the table's one buffer descriptor (the launcher's
// gate: the table is shorter than 4 GiB). Each lane adds its item's slots in
// slot order from zero (ACCUM: from the running row): the chain of
// gspmm_sum_kernel, so the same bits. Slots that only the longer item has run
// with the shorter half's lanes switched off: nothing fetched, nothing added
// (not even a zero: -0.0 + 0.0 is +0.0). An odd item count ends on a wave whose upper half is off. Running
// rows as RP 2 (ACCUM) / RP 4 of the one-item kernel, 16 bytes per lane.
template <int DEPTH, bool ACCUM>
__global__ __launch_bounds__(256) void gspmm_items_pair_kernel(
    int64_t num_items, int64_t ldu, uint32_t table_bytes,
    const int32_t* __restrict__ indices, const float* __restrict__ ufeat,
    float* __restrict__ out, const int32_t* __restrict__ item_rows,
    const int64_t* __restrict__ item_ptr) {
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  constexpr int64_t F = 128;
  const int lane = threadIdx.x & 63;
  const int64_t wave =
      block_linear() * (blockDim.x >> 6) +
      __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int64_t i0 = wave * 2;
  if (i0 >= num_items) return;
  const bool two = i0 + 1 < num_items;  // uniform
  const bool hi = lane >= 32;
  // slots [b0, b1) into row r0, [b1, e1) into row r1
  const int64_t b0 = item_ptr[i0], b1 = item_ptr[i0 + 1];
  const int64_t e1 = two ? item_ptr[i0 + 2] : b1;
  const int64_t r0 = item_rows[i0];
  const int64_t r1 = two ? item_rows[i0 + 1] : r0;
  const int n0 = static_cast<int>(b1 - b0), n1 = static_cast<int>(e1 - b1);
  const int nmin = n0 < n1 ? n0 : n1, nmax = n0 < n1 ? n1 : n0;
  const int32_t* __restrict__ idx0 = indices + b0;
  const int32_t* __restrict__ idx1 = indices + b1;
  const uint32_t ld4 = static_cast<uint32_t>(ldu) * 4u;
  const uint32_t lane_off = static_cast<uint32_t>(lane & 31) * 16u;
  const __amdgpu_buffer_rsrc_t table = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(ufeat), 0, static_cast<int>(table_bytes), 0x00020000);
  const int64_t f0 = int64_t(lane & 31) * 4;
  float* const orow = out + (hi ? r1 : r0) * F;
  const bool owns = !hi || two;

  f32x4 acc = Vec<4>::zero();
  if (ACCUM && owns) acc = load_out<4, 2>(orow, f0);
  int k = 0;
  // both items have DEPTH slots left: every lane gathers, no predicate
#pragma unroll 1
  for (; k + DEPTH <= nmin; k += DEPTH) {
    u32x4 v[DEPTH];
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) {
      const uint32_t o0 = static_cast<uint32_t>(idx0[k + j]) * ld4;
      const uint32_t o1 = static_cast<uint32_t>(idx1[k + j]) * ld4;
      v[j] = __builtin_amdgcn_raw_buffer_load_b128(table, (hi ? o1 : o0) + lane_off, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) acc += *reinterpret_cast<const f32x4*>(&v[j]);
  }
  // the rest as predicated batches, every gather of a batch in flight
  // together. A lane whose item has no slot k + j is switched off for it: its
  // gather goes to an offset past the table, which the descriptor's range
  // check answers without a fetch, and the value is not added. The scalar
  // column loads stay inside the pair's slots (an ended item re-reads its
  // last id, an empty one the other item's).
  const int my_n = hi ? n1 : n0;
  const int32_t* __restrict__ tail0 = n0 > 0 ? idx0 : idx1;
  const int32_t* __restrict__ tail1 = n1 > 0 ? idx1 : idx0;
  const int last0 = n0 > 0 ? n0 - 1 : n1 - 1, last1 = n1 > 0 ? n1 - 1 : n0 - 1;
#pragma unroll 1
  for (; k < nmax; k += DEPTH) {
    const int rb = nmax - k;
    u32x4 v[DEPTH];
    int32_t c0[DEPTH], c1[DEPTH];
    // the batch's ids first, all in flight: one scalar round trip, not one
    // ahead of every gather (the empty asm keeps the compiler from sinking
    // each load to its use)
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) {
      c0[j] = tail0[k + j < last0 ? k + j : last0];
      c1[j] = tail1[k + j < last1 ? k + j : last1];
    }
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) asm volatile("" : "+s"(c0[j]), "+s"(c1[j]));
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) {
      if (j < rb) {  // uniform
        const uint32_t o0 = static_cast<uint32_t>(c0[j]) * ld4;
        const uint32_t o1 = static_cast<uint32_t>(c1[j]) * ld4;
        const uint32_t off = k + j < my_n ? (hi ? o1 : o0) + lane_off : 0xfffffff0u;
        v[j] = __builtin_amdgcn_raw_buffer_load_b128(table, off, 0, 0);
      }
    }
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) {
      if (j < rb) {
        const f32x4 sum = acc + *reinterpret_cast<const f32x4*>(&v[j]);
        acc = k + j < my_n ? sum : acc;
      }
    }
  }
  // one store per half: the row of a half is uniform, as store_out's
  // descriptor has to be
  if (!hi) store_out<4, ACCUM ? 2 : 4>(out + r0 * F, f0, acc);
  else if (two) store_out<4, ACCUM ? 2 : 4>(out + r1 * F, f0, acc);
}

// Lane j of every 16-lane row (a DPP row) handed to the whole row.
__device__ __forceinline__ uint32_t row_broadcast(uint32_t v, int j) {
  switch (j) {
#define DGLHIP_ROW_BCAST(J) \
  case J: return __builtin_amdgcn_update_dpp(0, v, 0x150 + J, 0xf, 0xf, true);
    DGLHIP_ROW_BCAST(0) DGLHIP_ROW_BCAST(1) DGLHIP_ROW_BCAST(2) DGLHIP_ROW_BCAST(3)
    DGLHIP_ROW_BCAST(4) DGLHIP_ROW_BCAST(5) DGLHIP_ROW_BCAST(6) DGLHIP_ROW_BCAST(7)
    DGLHIP_ROW_BCAST(8) DGLHIP_ROW_BCAST(9) DGLHIP_ROW_BCAST(10) DGLHIP_ROW_BCAST(11)
    DGLHIP_ROW_BCAST(12) DGLHIP_ROW_BCAST(13) DGLHIP_ROW_BCAST(14)
#undef DGLHIP_ROW_BCAST
    default: return __builtin_amdgcn_update_dpp(0, v, 0x15f, 0xf, 0xf, true);
  }
}

// Column halves: four items per wave over one half of the columns, for the
// launches of gspmm_items_pair_kernel (DESIGN.md §4.1 "Column halves"). A
// workgroup gathers only columns [64 * half, 64 * half + 64) of every source
// row, half = (block % 8) & 1: blocks b and b + 8 share an XCD, so each XCD's
// L2 holds one half of the launch's source slice instead of all of it. The
// label is for speed only: block b takes half b & 1 of item group b >> 1 (16
// items), a bijection onto all the work wherever the block runs. Wave w of a
// group takes items 4w .. 4w + 3, one per quarter (16 lanes, a DPP row, 16
// bytes per lane), so one gather instruction still fetches 1 KiB: four half
// rows. The column ids of a batch come from one vector load, lane 16t + j
// reading item t's slot k + j and turning it into the row's byte offset (or,
// past the item's end, an offset past the table, which the descriptor's
// range check answers without a fetch); a row broadcast hands slot j's offset
// to its quarter. Each lane adds its item's slots in slot order from zero
// (ACCUM: from the running row) and a switched-off lane adds nothing: the
// chain of gspmm_sum_kernel, the same bits.
// A wave's round trips other than its gathers are kept off its critical path
// (DESIGN.md §4.1 "Column halves", the wave schedule): the nine item records
// come in one scalar trip; the first ids leave ahead of the running row; the
// next batch's ids are loaded behind the gathers and looked at only after the
// batch's adds; the four rows leave in one store. Exactly 64 VGPRs (8 waves
// per SIMD): the kernel is compiled for that occupancy, check the resource
// usage for scratch after any change.
template <int DEPTH, bool ACCUM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void
gspmm_items_columns_kernel(
    int64_t num_items, int64_t ldu, uint32_t table_bytes, uint32_t out_bytes,
    const int32_t* __restrict__ indices, const float* __restrict__ ufeat,
    float* __restrict__ out, const int32_t* __restrict__ item_rows,
    const int64_t* __restrict__ item_ptr) {
  static_assert(DEPTH >= 1 && DEPTH <= 16, "a batch's ids are one 16-lane row");
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  constexpr uint32_t kOff = 0xfffffc00u;  // + any lane offset: past every gated table
  const int lane = threadIdx.x & 63;
  const int q = lane >> 4, ql = lane & 15;
  const int64_t bl = block_linear();
  const int half = static_cast<int>(bl % 8) & 1;
  const int64_t wave =
      (bl >> 1) * (blockDim.x >> 6) +
      __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int64_t i0 = wave * 4;
  if (i0 >= num_items) return;
  // quarter t: slots [p[t], p[t + 1]) into row r[t]
  int64_t p[5];
  int64_t r[4];
  if (i0 + 4 <= num_items) {  // uniform: every wave but, at most, the launch's last
    // the nine records in one scalar round trip: wide loads (the arrays are
    // only element-aligned) with nothing between them to wait for
    typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
    typedef int64_t i64x4 __attribute__((ext_vector_type(4)));
    typedef i32x4 i32x4_a4 __attribute__((aligned(4)));
    typedef i64x4 i64x4_a8 __attribute__((aligned(8)));
    const i32x4 rr = *reinterpret_cast<const i32x4_a4*>(item_rows + i0);
    const i64x4 pp = *reinterpret_cast<const i64x4_a8*>(item_ptr + i0);
    p[4] = item_ptr[i0 + 4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      p[t] = pp[t];
      r[t] = rr[t];
    }
  } else {
    // the last wave: none past the last item (a dead quarter has no slots and
    // the last item's row)
#pragma unroll
    for (int t = 0; t < 5; ++t) p[t] = item_ptr[i0 + t < num_items ? i0 + t : num_items];
#pragma unroll
    for (int t = 0; t < 4; ++t) r[t] = item_rows[i0 + t < num_items ? i0 + t : num_items - 1];
  }
  int n[4], rel[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    n[t] = static_cast<int>(p[t + 1] - p[t]);
    rel[t] = static_cast<int>(p[t] - p[0]);
  }
  const int nmin = min(min(n[0], n[1]), min(n[2], n[3]));
  const int nmax = max(max(n[0], n[1]), max(n[2], n[3]));
  const int my_n = q == 0 ? n[0] : (q == 1 ? n[1] : (q == 2 ? n[2] : n[3]));
  const int my_rel = q == 0 ? rel[0] : (q == 1 ? rel[1] : (q == 2 ? rel[2] : rel[3]));
  const uint32_t ld4 = static_cast<uint32_t>(ldu) * 4u;
  const uint32_t lane_off = static_cast<uint32_t>(half) * 256u + static_cast<uint32_t>(ql) * 16u;
  const __amdgpu_buffer_rsrc_t table = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(ufeat), 0, static_cast<int>(table_bytes), 0x00020000);
  // the wave's slots behind a descriptor: a 32-bit offset per id load
  const __amdgpu_buffer_rsrc_t slots = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<int32_t*>(indices + p[0]), 0, 0x7fffffff, 0x00020000);
  // all of out behind one (the gate: shorter than 4 GiB): lane ln's 16 bytes
  // of its quarter's row
  const __amdgpu_buffer_rsrc_t rows = __builtin_amdgcn_make_buffer_rsrc(
      out, 0, static_cast<int>(out_bytes), 0x00020000);
  auto row_offset = [&](int ln) -> uint32_t {
    const int t = ln >> 4;
    const int64_t row = t == 0 ? r[0] : (t == 1 ? r[1] : (t == 2 ? r[2] : r[3]));
    return static_cast<uint32_t>(row) * 512u + static_cast<uint32_t>(half) * 256u +
           static_cast<uint32_t>(ln & 15) * 16u;
  };

  // this lane's share of the batch at slot k: the id of slot k + ql of its
  // quarter's item, then the byte offset of that row (past the item's end:
  // past the table). The load stays inside the wave's slots (an ended item
  // re-reads its last id, an empty one a neighbour's), so it needs no
  // predicate, also for a batch that does not come.
  auto load_ids = [&](int k) -> uint32_t {
    const int s = max(min(k + ql, my_n - 1) + my_rel, 0);
    return __builtin_amdgcn_raw_buffer_load_b32(slots, static_cast<uint32_t>(s) * 4u, 0, 0);
  };
  auto offsets = [&](uint32_t id, int k) -> uint32_t { return k + ql < my_n ? id * ld4 : kOff; };
  // the running row, non-temporal (RP 2 of load_out). A dead quarter reads the
  // last item's row and stores nothing.
  auto load_row = [&]() -> f32x4 {
    const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(rows, row_offset(lane), 0, 2);
    return *reinterpret_cast<const f32x4*>(&w);
  };

  f32x4 acc = Vec<4>::zero();
  if (nmax > 0) {
    // the first ids leave ahead of the running row, which comes from the
    // fabric and is not needed before the first add: the gathers wait for the
    // ids alone. (Vector loads return in order. The barriers keep the
    // compiler's scheduler from swapping the two; the empty asm is the first
    // use of the ids, where the wait goes.)
    uint32_t raw = load_ids(0);
    __builtin_amdgcn_sched_barrier(0);
    if (ACCUM) acc = load_row();
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" : "+v"(raw));
    uint32_t ids = offsets(raw, 0);
    int k = 0;
    // every item has DEPTH slots left: every lane gathers, no predicate
#pragma unroll 1
    for (; k + DEPTH <= nmin; k += DEPTH) {
      u32x4 v[DEPTH];
#pragma unroll
      for (int j = 0; j < DEPTH; ++j)
        v[j] = __builtin_amdgcn_raw_buffer_load_b128(table, row_broadcast(ids, j) + lane_off, 0,
                                                     0);
      // the next batch's ids behind the gathers, not looked at before the
      // batch's last add: each add waits for its own gather only, and the id
      // round trip (a first touch, from the fabric) runs beside the chain
      raw = load_ids(k + DEPTH);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < DEPTH; ++j) acc += *reinterpret_cast<const f32x4*>(&v[j]);
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("" : "+v"(raw));
      ids = offsets(raw, k + DEPTH);
    }
    // the rest as predicated batches, every gather of a batch in flight
    // together; a lane whose item has no slot k + j gathers past the table and
    // does not add the value (not even a zero: -0.0 + 0.0 is +0.0)
#pragma unroll 1
    for (; k < nmax; k += DEPTH) {
      const int rb = nmax - k;
      u32x4 v[DEPTH];
#pragma unroll
      for (int j = 0; j < DEPTH; ++j) {
        if (j < rb)  // uniform
          v[j] = __builtin_amdgcn_raw_buffer_load_b128(table, row_broadcast(ids, j) + lane_off,
                                                       0, 0);
      }
      raw = load_ids(k + DEPTH);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < DEPTH; ++j) {
        if (j < rb) {
          const f32x4 sum = acc + *reinterpret_cast<const f32x4*>(&v[j]);
          acc = k + j < my_n ? sum : acc;
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("" : "+v"(raw));
      ids = offsets(raw, k + DEPTH);
    }
  } else if (ACCUM) {
    acc = load_row();
  }
  // one store for the wave's four rows (sc1: the lines leave the XCD's L2, RP
  // 2 / 4 of store_out), the quarters past the last item switched off. The
  // lane's place is worked out again from its id in the wave: held across the
  // batches it would be the 65th register.
  const int ln = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  if (i0 + (ln >> 4) < num_items)
    __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4*>(&acc), rows,
                                           row_offset(ln), 0, 16);
}

// Combine the chunk partials of each heavy row in chunk order:
// out[row] = ((p0 + p1) + p2) + ... (deterministic), then MEAN scaling; with
// ACCUM the row's running value comes first: out[row] = ((out[row] + p0) + p1) ...;
// with MEAN and ACCUM the mean is added to it: out[row] + (p0 + p1 + ...) / deg
template <bool MEAN, bool ACCUM>
__global__ __launch_bounds__(256) void gspmm_combine_kernel(
    int64_t num_heavy, int64_t F, const int64_t* __restrict__ indptr,
    const int32_t* __restrict__ heavy_rows, const int64_t* __restrict__ heavy_chunk_ptr,
    const float* __restrict__ partial, float* __restrict__ out) {
  const int64_t wave = block_linear() * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (wave >= num_heavy) return;
  const int lane = threadIdx.x & 63;
  const int64_t row = heavy_rows[wave];
  const int64_t c0 = heavy_chunk_ptr[wave], c1 = heavy_chunk_ptr[wave + 1];
  const float deg = static_cast<float>(indptr[row + 1] - indptr[row]);
  for (int64_t f = lane; f < F; f += 64) {
    float acc = (ACCUM && !MEAN) ? out[row * F + f] + partial[c0 * F + f] : partial[c0 * F + f];
    for (int64_t c = c0 + 1; c < c1; ++c) acc += partial[c * F + f];
    if (MEAN && deg > 1.0f) acc = acc / deg;
    if (MEAN && ACCUM) acc = out[row * F + f] + acc;
    out[row * F + f] = acc;
  }
}

// Max-reduce kernel with argmax slot: first slot wins ties (a strict running
// max over the mailbox, seeded with the first message), and a NaN message is
// taken like a larger one and then kept (torch.max: the row's first NaN wins,
// value and argmax; segment_reduce.hip's max_step is the same rule); 0 / -1
// for rows without slots. Same lane mapping as the sum kernel (GROUP lanes
// per row, VEC features per lane, UNROLL gathers in flight); the compares
// then run slot by slot in CSR order, so the argmax is the one the sequential
// reduction picks. A NaN running value is never replaced, so a row continued
// from an earlier source block (prev) keeps the earlier block's NaN.
// The rule is "best is not NaN, and x is greater or NaN"; !(x <= best) is
// "greater or unordered", and the mask AND keeps it two compares without the
// per-element branches a short-circuit && / || compiles to.
__device__ __forceinline__ bool max_takes(float x, float best) {
  return (best == best) & !(x <= best);
}

template <int VEC, int UNROLL, int MSG, int EM, bool USE_EID>
__device__ __forceinline__ void max_row(int64_t row, int gl, int group, int64_t beg,
                                        int64_t end, int64_t F, int64_t elen,
                                        const int32_t* __restrict__ indices,
                                        const int64_t* __restrict__ eid,
                                        const float* __restrict__ ufeat,
                                        const float* __restrict__ efeat,
                                        float* __restrict__ out, int64_t* __restrict__ arg_out,
                                        bool prev = false) {
  typedef typename Vec<VEC>::T V;
  auto message = [](const SlotLoad<VEC, MSG, EM>& s) -> V {
    if (copies_u(MSG)) return s.u;
    if (MSG == DGLHIP_MSG_COPY_E) return s.e;
    return s.u * s.e;
  };
  auto edge = [&](int64_t k) -> int64_t {
    return copies_u(MSG) ? 0 : (USE_EID ? eid[k] : k);
  };
  for (int64_t f0 = int64_t(gl) * VEC; f0 < F; f0 += int64_t(group) * VEC) {
    const int64_t eoff = EM == EM_HEAD ? f0 / (F / elen) : (EM == EM_FULL ? f0 : 0);
    V best = Vec<VEC>::zero();
    int64_t arg[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) arg[i] = -1;
    int64_t k = beg;
    if (prev) {  // the row's earlier slots (a previous source block): continue from them
      best = ldv<VEC>(out + row * F + f0);
#pragma unroll
      for (int i = 0; i < VEC; ++i) arg[i] = arg_out ? arg_out[row * F + f0 + i] : -1;
    } else if (k < end) {
      SlotLoad<VEC, MSG, EM> s;
      s.load(ufeat, efeat, F, F, f0, elen, eoff, indices[k], edge(k));
      best = message(s);
#pragma unroll
      for (int i = 0; i < VEC; ++i) arg[i] = k;
      ++k;
    }
    for (; k + UNROLL <= end; k += UNROLL) {
      SlotLoad<VEC, MSG, EM> s[UNROLL];
#pragma unroll
      for (int j = 0; j < UNROLL; ++j)
        s[j].load(ufeat, efeat, F, F, f0, elen, eoff, indices[k + j], edge(k + j));
#pragma unroll
      for (int j = 0; j < UNROLL; ++j) {
        const V x = message(s[j]);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const float xi = reinterpret_cast<const float*>(&x)[i];
          float& bi = reinterpret_cast<float*>(&best)[i];
          if (max_takes(xi, bi)) { bi = xi; arg[i] = k + j; }
        }
      }
    }
    const int64_t rem = end - k;  // the last < UNROLL slots: one predicated batch
    if (rem > 0) {
      SlotLoad<VEC, MSG, EM> s[UNROLL];
#pragma unroll
      for (int j = 0; j < UNROLL - 1; ++j)
        if (j < rem) s[j].load(ufeat, efeat, F, F, f0, elen, eoff, indices[k + j], edge(k + j));
#pragma unroll
      for (int j = 0; j < UNROLL - 1; ++j) {
        if (j < rem) {
          const V x = message(s[j]);
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            const float xi = reinterpret_cast<const float*>(&x)[i];
            float& bi = reinterpret_cast<float*>(&best)[i];
            if (max_takes(xi, bi)) { bi = xi; arg[i] = k + j; }
          }
        }
      }
    }
    stv<VEC>(out + row * F + f0, best);
    if (arg_out) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) arg_out[row * F + f0 + i] = arg[i];
    }
  }
}

template <int VEC, int GROUP, int UNROLL, int MSG, int EM>
__global__ __launch_bounds__(256) void gspmm_max_kernel(
    int64_t num_rows, int64_t F, int64_t elen, const int64_t* __restrict__ indptr,
    const int32_t* __restrict__ indices, const int64_t* __restrict__ eid,
    const float* __restrict__ ufeat, const float* __restrict__ efeat,
    float* __restrict__ out, int64_t* __restrict__ arg_out,
    const int32_t* __restrict__ row_order, const int64_t* __restrict__ row_beg,
    const int64_t* __restrict__ row_end, int accumulate) {
  constexpr int ITEMS_PER_WAVE = 64 / GROUP;
  const int lane = threadIdx.x & 63;
  const int64_t wave =
      block_linear() * (blockDim.x >> 6) +
      __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int64_t it = wave * ITEMS_PER_WAVE + (GROUP == 64 ? 0 : lane / GROUP);
  if (it >= num_rows) return;
  const int gl = GROUP == 64 ? lane : (lane % GROUP);
  int64_t row = row_order ? row_order[it] : it;
  if (GROUP == 64) row = __builtin_amdgcn_readfirstlane(static_cast<int>(row));
  // row ranges (source-blocked schedule): the row's slots [row_beg, row_end)
  // of this block; with accumulate, continue from the earlier blocks' max
  const int64_t rs = indptr[row];
  const int64_t beg = row_beg ? row_beg[row] : rs;
  const int64_t end = row_end ? row_end[row] : indptr[row + 1];
  if (accumulate && beg == end) return;  // nothing new: the row keeps its value
  const bool prev = accumulate && beg > rs;
  if (copies_u(MSG) || eid != nullptr)  // uniform branch
    max_row<VEC, UNROLL, MSG, EM, true>(row, gl, GROUP, beg, end, F, elen, indices, eid, ufeat,
                                        efeat, out, arg_out, prev);
  else
    max_row<VEC, UNROLL, MSG, EM, false>(row, gl, GROUP, beg, end, F, elen, indices, eid,
                                         ufeat, efeat, out, arg_out, prev);
}

// ---------------------------------------------------------------------------
// Dispatch
// ---------------------------------------------------------------------------
// Widest per-lane vector the row length and every feature pointer allow.
static inline int pick_vec(int64_t F, std::initializer_list<const void*> ptrs) {
  auto aligned = [&](int bytes) {
    for (const void* p : ptrs)
      if (p && (reinterpret_cast<uintptr_t>(p) % bytes) != 0) return false;
    return true;
  };
  // no VEC 4: at F=256 one 1-KB row per wave instruction (8 gathers
  // in flight) ran 16.3 ms against 15.7 ms for two VEC-2 passes with 16 in
  // flight (profiles/r01/feat_sweep_reddit.json, Reddit-shaped graph)
  if (F % 2 == 0 && F >= 4 && aligned(8)) return 2;
  return 1;
}

static inline int pick_group(int64_t F, int vec) {
  const int64_t lanes = (F + vec - 1) / vec;
  int g = 1;
  while (g < lanes && g < 64) g <<= 1;
  return g;
}

// Rows of 16..64 floats take a whole wave each (idle lanes) rather than
// sharing one: the slot stream is then wave-uniform (column ids through the
// scalar cache) instead of a per-lane index load ahead of every gather.
// profiles/r01/feat_sweep_reddit.json, Reddit-shaped graph: F=16 2.18 -> 1.73 ms, F=32
// 2.12 -> 1.74 ms, F=64 level.
static inline void one_row_per_wave(int64_t F, int& vec, int& group) {
  if (group < 64 && F >= 16) {
    vec = 1;
    group = 64;
  }
}

struct SumLaunch {
  int64_t num_items, F, elen;
  const int64_t* indptr;
  const int32_t* indices;
  const int64_t* eid;
  const float* ufeat;
  const float* efeat;
  float* out;
  const int32_t* row_order;
  const int64_t* chunk_beg;  // non-null: chunked launch (partials to `out`)
  const int64_t* chunk_end;
  bool accumulate;           // continue each item's chain from the value in `out`
  bool nt_out = false;       // non-temporal output stores (see stream_output)
  int64_t ldu = 0;           // ufeat row stride in elements (0: F)
  int64_t urows = 0;         // rows of ufeat (0: not known)
  int items_per_wave = 1;    // 2: gspmm_items_pair_kernel where it applies
  int column_parts = 1;      // 2: gspmm_items_columns_kernel where it applies
  int64_t orows = 0;         // rows of out (0: not known)
};

// Outputs past twice the 256 MiB Infinity Cache are stored non-temporally
// (POL_NT_OUT): streamed out, they would evict the feature rows that are
// gathered again (RMAT-26, 34 GB out: 94.1 -> 89.5 ms, DESIGN.md, the r01
// cache-policy study). Covers copy_u + sum at VEC 2 x 64 lanes.
static inline bool stream_output(int64_t rows, int64_t feat_len) {
  return rows * feat_len * int64_t(sizeof(float)) > (int64_t(512) << 20);
}

// Whether a copy_u launch of the blocked schedule's items takes the two-
// items-per-wave kernel: fp32 rows of 128 floats, 16-byte lanes (the table,
// its row stride and out aligned to them) and 32-bit gather offsets (the
// table shorter than 4 GiB, which needs its row count).
static inline bool items_pair_applies(const SumLaunch& a) {
  const int64_t ldu = a.ldu ? a.ldu : a.F;
  return a.items_per_wave == 2 && a.F == 128 && a.urows > 0 && ldu % 4 == 0 &&
         reinterpret_cast<uintptr_t>(a.ufeat) % 16 == 0 &&
         reinterpret_cast<uintptr_t>(a.out) % 16 == 0 &&
         a.urows * ldu * int64_t(sizeof(float)) < (int64_t(1) << 32);
}

// Whether it takes the column-half kernel instead: the pair kernel's gate,
// and a table that ends 1 KiB below 4 GiB (a switched-off lane's offset plus
// its column offset must neither wrap nor fall inside the table), and 32-bit
// offsets into out for the wave's one store: out shorter than 4 GiB, which
// needs its row count.
static inline bool items_columns_applies(const SumLaunch& a) {
  const int64_t ldu = a.ldu ? a.ldu : a.F;
  return a.column_parts == 2 && items_pair_applies(a) &&
         a.urows * ldu * int64_t(sizeof(float)) <= int64_t(0xfffffc00u) && a.orows > 0 &&
         a.orows * a.F * int64_t(sizeof(float)) < (int64_t(1) << 32);
}

static inline void launch_items_columns(const SumLaunch& a, hipStream_t stream) {
  // 12 gathers in flight per lane: the most that keep 64 VGPRs, so 8 waves per
  // SIMD (8 / 10 / 12 / 14 / 16 measured: DESIGN.md §4.1 "Column halves")
  constexpr int DEPTH = 12;
  // 16 items (4 waves of 4) per pair of blocks, one block per column half
  const int64_t blocks = 2 * ((a.num_items + 15) / 16);
  DGLHIP_CHECK(blocks <= 0x7fffffff, "grid too large: " << blocks);
  const int64_t ldu = a.ldu ? a.ldu : a.F;
  auto kernel = a.accumulate ? gspmm_items_columns_kernel<DEPTH, true>
                             : gspmm_items_columns_kernel<DEPTH, false>;
  timed_launch(stream, [&] {
    hipLaunchKernelGGL(kernel, grid_1d(blocks), dim3(256), 0, stream, a.num_items, ldu,
                       static_cast<uint32_t>(a.urows * ldu * int64_t(sizeof(float))),
                       static_cast<uint32_t>(a.orows * a.F * int64_t(sizeof(float))), a.indices,
                       a.ufeat, a.out, a.row_order, a.chunk_beg);
  });
}

static inline void launch_items_pair(const SumLaunch& a, hipStream_t stream) {
  // 10 pairs of rows in flight per wave: the most that keep 64 VGPRs, so 8
  // waves per SIMD (8 / 10 / 12 / 16 measured: DESIGN.md §4.1 "Two items per wave")
  constexpr int DEPTH = 10;
  const int64_t blocks = (a.num_items + 7) / 8;  // 4 waves of 2 items
  DGLHIP_CHECK(blocks <= 0x7fffffff, "grid too large: " << blocks);
  const int64_t ldu = a.ldu ? a.ldu : a.F;
  auto kernel = a.accumulate ? gspmm_items_pair_kernel<DEPTH, true>
                             : gspmm_items_pair_kernel<DEPTH, false>;
  timed_launch(stream, [&] {
    hipLaunchKernelGGL(kernel, grid_1d(blocks), dim3(256), 0, stream, a.num_items, ldu,
                       static_cast<uint32_t>(a.urows * ldu * int64_t(sizeof(float))), a.indices,
                       a.ufeat, a.out, a.row_order, a.chunk_beg);
  });
}

template <int VEC, int GROUP, int MSG, int EM, bool MEAN>
static inline void launch_sum(const SumLaunch& a, hipStream_t stream) {
  // 16 row gathers in flight per lane group: measured +22% over 8 on HBM-bound
  // RMAT, neutral on the MALL-resident Reddit table
  constexpr int UNROLL = 16;
  constexpr int ITEMS_PER_BLOCK = 4 * (64 / GROUP);
  const int64_t blocks = (a.num_items + ITEMS_PER_BLOCK - 1) / ITEMS_PER_BLOCK;
  DGLHIP_CHECK(blocks <= 0x7fffffff, "grid too large: " << blocks);
  if (blocks == 0) return;
  const bool chunked = a.chunk_beg != nullptr;
  // every instantiation has one signature: choose the kernel, then launch it
  auto kernel = gspmm_sum_kernel<VEC, GROUP, UNROLL, MSG, EM, MEAN, false, false>;
  if (chunked && a.accumulate)
    kernel = gspmm_sum_kernel<VEC, GROUP, UNROLL, MSG, EM, MEAN, true, true>;
  else if (chunked)
    kernel = gspmm_sum_kernel<VEC, GROUP, UNROLL, MSG, EM, MEAN, true, false>;
  else if (a.accumulate)
    kernel = gspmm_sum_kernel<VEC, GROUP, UNROLL, MSG, EM, MEAN, false, true>;
  // copy_u + sum with a whole wave of two-float lanes per row (F = 128 and
  // wider): the one shape with an output policy, buffer-descriptor gathers
  // and a running-row policy
  constexpr bool POL_OK = MSG == DGLHIP_MSG_COPY_U && VEC == 2 && GROUP == 64 && !MEAN;
  if constexpr (POL_OK) {
    if (chunked && a.row_order && !a.nt_out) {
      // the blocked schedule's items (item rows given; heavy-row chunk and
      // row-range launches keep the generic kernels: r04 ADVICE). Row gathers
      // through per-row buffer descriptors (the row base in SGPRs, one lane
      // offset for all 16: 42 instead of 70 VGPRs, 8 waves per SIMD instead of
      // 7; Reddit-shaped headline 3.74 -> 3.61 ms, same bits); the running
      // rows under RP 2, the first launch, which only stores, under RP 4.
      // With items_per_wave 2, rows of 128 floats go two items to a wave.
      // With column_parts 2 on top, four items to a wave over a column half.
      if (items_columns_applies(a)) {
        launch_items_columns(a, stream);
        return;
      }
      if (items_pair_applies(a)) {
        launch_items_pair(a, stream);
        return;
      }
      if (a.accumulate)
        kernel = gspmm_sum_kernel<VEC, GROUP, UNROLL, MSG, EM, false, true, true, POL_DEFAULT,
                                  true, 2>;
      else
        kernel = gspmm_sum_kernel<VEC, GROUP, UNROLL, MSG, EM, false, true, false, POL_DEFAULT,
                                  true, 4>;
    } else if (a.nt_out && !a.accumulate) {
      // an output past twice the Infinity Cache (stream_output)
      if (chunked)
        kernel = gspmm_sum_kernel<VEC, GROUP, UNROLL, MSG, EM, false, true, false, POL_NT_OUT>;
      else
        kernel = gspmm_sum_kernel<VEC, GROUP, UNROLL, MSG, EM, false, false, false, POL_NT_OUT>;
    }
  }
  timed_launch(stream, [&] {
    hipLaunchKernelGGL(kernel, grid_1d(blocks), dim3(256), 0, stream, a.num_items, a.F, a.elen,
                       a.ldu ? a.ldu : a.F, a.indptr, a.indices, a.eid, a.ufeat, a.efeat, a.out,
                       a.row_order, a.chunk_beg, a.chunk_end);
  });
}

template <int MSG, int EM, bool MEAN>
static inline void dispatch_sum_shape(const SumLaunch& a, hipStream_t stream) {
  const int64_t F = a.F;
  int vec = pick_vec(F, {a.ufeat, EM == EM_FULL ? a.efeat : nullptr, a.out});
  // per-head weights: a lane's VEC features must stay inside one head
  while (EM == EM_HEAD && vec > 1 && (F / a.elen) % vec != 0) vec >>= 1;
  int group = pick_group(F, vec);
  one_row_per_wave(F, vec, group);
#define DGLHIP_CASE(V, G)                                  \
  if (vec == V && group == G) {                            \
    launch_sum<V, G, MSG, EM, MEAN>(a, stream);            \
    return;                                                \
  }
  DGLHIP_CASE(2, 64) DGLHIP_CASE(2, 32) DGLHIP_CASE(2, 16) DGLHIP_CASE(2, 8)
  DGLHIP_CASE(2, 4) DGLHIP_CASE(2, 2)
  DGLHIP_CASE(1, 64) DGLHIP_CASE(1, 32) DGLHIP_CASE(1, 16) DGLHIP_CASE(1, 8)
  DGLHIP_CASE(1, 4) DGLHIP_CASE(1, 2) DGLHIP_CASE(1, 1)
#undef DGLHIP_CASE
  DGLHIP_CHECK(false, "no kernel for F=" << F << " vec=" << vec << " group=" << group);
}

static inline int edge_mode(int64_t elen, int64_t F) {
  return elen == F ? EM_FULL : (elen == 1 ? EM_SCALAR : EM_HEAD);
}


struct MaxLaunch {
  int64_t num_rows, F, elen;
  const int64_t* indptr;
  const int32_t* indices;
  const int64_t* eid;
  const float* ufeat;
  const float* efeat;
  float* out;
  int64_t* arg_out;
  const int32_t* row_order;
  const int64_t* row_beg = nullptr;  // row ranges (NULL: whole rows)
  const int64_t* row_end = nullptr;
  int accumulate = 0;
};


template <int MSG, int EM>
static inline void dispatch_max_shape(const MaxLaunch& a, hipStream_t stream) {
  const int64_t F = a.F;
  int vec = pick_vec(F, {a.ufeat, EM == EM_FULL ? a.efeat : nullptr, a.out});
  while (EM == EM_HEAD && vec > 1 && (F / a.elen) % vec != 0) vec >>= 1;
  int group = pick_group(F, vec);
  one_row_per_wave(F, vec, group);
#define DGLHIP_CASE(V, G)                                                            \
  if (vec == V && group == G) {                                                      \
    constexpr int ITEMS_PER_BLOCK = 4 * (64 / G);                                    \
    const int64_t blocks = (a.num_rows + ITEMS_PER_BLOCK - 1) / ITEMS_PER_BLOCK;     \
    DGLHIP_CHECK(blocks <= 0x7fffffff, "grid too large: " << blocks);                \
    timed_launch(stream, [&] {                                                       \
      hipLaunchKernelGGL((gspmm_max_kernel<V, G, 8, MSG, EM>),                       \
                         grid_1d(blocks), dim3(256), 0, stream,  \
                         a.num_rows, a.F, a.elen, a.indptr, a.indices, a.eid,        \
                         a.ufeat, a.efeat, a.out, a.arg_out, a.row_order, a.row_beg, \
                         a.row_end, a.accumulate);                                   \
    });                                                                              \
    return;                                                                          \
  }
  DGLHIP_CASE(2, 64) DGLHIP_CASE(2, 32) DGLHIP_CASE(2, 16) DGLHIP_CASE(2, 8)
  DGLHIP_CASE(2, 4) DGLHIP_CASE(2, 2)
  DGLHIP_CASE(1, 64) DGLHIP_CASE(1, 32) DGLHIP_CASE(1, 16) DGLHIP_CASE(1, 8)
  DGLHIP_CASE(1, 4) DGLHIP_CASE(1, 2) DGLHIP_CASE(1, 1)
#undef DGLHIP_CASE
  DGLHIP_CHECK(false, "no max kernel for F=" << F << " vec=" << vec << " group=" << group);
}


// One (message, edge layout) pair of the sum/mean and max reducers. Defined
// only in gspmm_inst.hip, which explicitly instantiates it per pair.
template <int MSG, int EM>
void dispatch_me(bool mean, const SumLaunch& a, hipStream_t stream);
template <int MSG, int EM>
void dispatch_me(const MaxLaunch& a, hipStream_t stream);

#ifdef GSPMM_INST_MSG
template <int MSG, int EM>
void dispatch_me(bool mean, const SumLaunch& a, hipStream_t stream) {
  if (mean) dispatch_sum_shape<MSG, EM, true>(a, stream);
  else dispatch_sum_shape<MSG, EM, false>(a, stream);
}
template <int MSG, int EM>
void dispatch_me(const MaxLaunch& a, hipStream_t stream) {
  dispatch_max_shape<MSG, EM>(a, stream);
}
#endif

}  // namespace dglhip
