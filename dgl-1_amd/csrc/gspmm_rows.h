// Row primitives of the g-SpMM kernels: the per-lane vectors, the row gathers
// and stores with their cache policies, one row's sequential reduction, the
// GAT dropout hash, and the host checks every g-SpMM entry point shares.
// Included by gspmm_impl.h (the generic reducers), gspmm_items.hip (the
// blocked schedule's item kernels), gat_fused.hip, short_rows.hip and
// sweep.hip. Design notes: gspmm.hip header and DESIGN.md §4.1.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

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

// Outputs past twice the 256 MiB Infinity Cache are stored non-temporally
// (POL_NT_OUT): streamed out, they would evict the feature rows that are
// gathered again (RMAT-26, 34 GB out: 94.1 -> 89.5 ms, DESIGN.md, the r01
// cache-policy study). Covers copy_u + sum at VEC 2 x 64 lanes.
static inline bool stream_output(int64_t rows, int64_t feat_len) {
  return rows * feat_len * int64_t(sizeof(float)) > (int64_t(512) << 20);
}

// The operand checks of every g-SpMM entry point: the tables the message
// reads are given, and an edge-feature row divides the feature row. Returns
// the edge-feature length the kernels take (1 where the message reads none).
static inline int64_t check_operands(int msg_op, int64_t feat_len, const float* ufeat,
                                     const float* efeat, int64_t efeat_len) {
  const bool use_u = msg_op != DGLHIP_MSG_COPY_E;
  const bool use_e = !copies_u(msg_op);
  DGLHIP_CHECK(!use_u || ufeat, "ufeat is null");
  DGLHIP_CHECK(!use_e || efeat, "efeat is null");
  DGLHIP_CHECK(!use_e || (efeat_len >= 1 && feat_len % efeat_len == 0),
               "edge feature length " << efeat_len << " must divide feat_len " << feat_len);
  return use_e ? efeat_len : 1;
}

// a lane's vector of VEC features must not straddle padded rows: even strides only
static inline void check_ufeat_ld(int64_t ufeat_ld, int64_t feat_len) {
  DGLHIP_CHECK(ufeat_ld == 0 || ufeat_ld == feat_len || (ufeat_ld > feat_len && ufeat_ld % 2 == 0),
               "ufeat_ld " << ufeat_ld << ": 0, feat_len, or an even width > feat_len");
}

// The blocked schedule's items on the generic sum kernel, one item per wave
// (gspmm.hip): what gspmm_items.hip launches where neither of its kernels
// applies. Operands checked by the caller; elen from check_operands.
void gspmm_items_one(int msg_op, int64_t num_items, int64_t feat_len, int64_t elen,
                     const int32_t* item_rows, const int64_t* item_ptr, bool accumulate,
                     const int32_t* indices, const int64_t* eid, const float* ufeat,
                     int64_t ufeat_ld, const float* efeat, float* out, hipStream_t stream);

}  // namespace dglhip
