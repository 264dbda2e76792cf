// The row walk and the softmax core of the fused attention kernels
// (dot_attention.hip, gatv2_attention.hip): what both units do with a CSR row
// whatever their score is, over the lane helpers of attention_lanes.h.
//
// Lane map, shared by every kernel of both units. A lane holds VEC
// consecutive features of one head (VEC = 4 with 16-byte accesses when
// D % 4 == 0 and every tensor is 16-byte aligned, else 2 with 8-byte ones,
// else 1). A head takes LPH lanes, the power of two that covers D / VEC (lanes
// past D idle, they hold zeros), a wave covers 64 / LPH heads, and more heads
// than that are further head tiles: a wave is one (row, head tile), since a
// head's softmax is its own. A dot product is summed per lane over its VEC
// features (one product, then fmas, in feature order) and then across the
// head's lanes by an xor butterfly: DPP at strides 1, 2 (quad permutes), 4, 8
// (the mirrors of 8 and 16 lanes: after the earlier stages a mirror's partner
// holds what the xor partner holds), __shfl_xor at 16 and 32. Both partners
// of a stage add the same two numbers, so every lane of a head ends with the
// same bits, and the walks of a unit compute the same bits for s_j: a clamp
// is active in all of them or in none.
//
// The walk. A wave takes up to 64 column ids of its row in one coalesced load
// and hands them out lane to lane; it runs the slots in batches of the unit's
// batch size: the batch's gathers are issued before first use, then the
// scores, then, in the forward, one rescale expf(m - m') of the running sum
// and the VEC accumulators per batch (m' the maximum of m and the batch's
// scores) and per slot, in slot order, p = expf(s - m'), l += p,
// acc = fma(p, v, acc) (softmax_step).
//
// Long rows. A row of more than a chunk of slots (the unit's
// DGLHIP_*_CHUNK, a template parameter here) is cut where it crosses the
// multiples of the chunk (row_pieces.h), a piece a wave. In the forward a
// piece leaves (m, l, acc[D]) per head in the workspace and the wave of the
// row's first piece merges them in block order (m = max m_g, weights
// expf(m_g - m)) and stores out and lse (fwd_combine); in the backward lse
// and delta are known, the pieces are plain partial sums, added in block
// order (sum_pieces).
//
// No atomics; every output element has one writer: the same bits on every call.
#pragma once

#include "attention_lanes.h"
#include "common.h"
#include "launch.h"
#include "row_pieces.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <initializer_list>
#include <type_traits>

namespace dglhip {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

// what every walk needs; a unit's Args derives from it
struct Walk {
  int64_t R, C, nnz, H, D;  // rows and columns of the CSR the kernel walks
  int64_t G;                // blocks of a chunk of slots (0: no row is longer than a chunk)
  int64_t tiles;            // head tiles per row
  int lph_shift;            // log2 of the lanes per head
  const int64_t* indptr;
  const int32_t* indices;
  const int32_t* row_order;
};

// a lane's place: VEC features of one head
struct Place {
  int64_t head;   // its head, and one that exists (for the loads of idle heads)
  int64_t hsafe;
  int64_t foff;   // head * D + its first feature
  bool live;      // it holds features
  bool first;     // the first lane of a head that exists
};

template <int VEC>
__device__ __forceinline__ Place place_of(const Walk& a, int64_t tile, int lane) {
  Place p;
  const int sub = lane & ((1 << a.lph_shift) - 1);
  p.head = tile * (64 >> a.lph_shift) + (lane >> a.lph_shift);
  const bool headok = p.head < a.H;
  p.hsafe = headok ? p.head : 0;
  p.live = headok && int64_t(sub) * VEC < a.D;
  p.first = headok && sub == 0;
  p.foff = p.head * a.D + int64_t(sub) * VEC;
  return p;
}

template <int VEC>
__device__ __forceinline__ void zero(float (&v)[VEC]) {
#pragma unroll
  for (int c = 0; c < VEC; ++c) v[c] = 0.0f;
}

// a lane's features of row `node` of a (nodes, H, D) tensor; zeros in idle lanes
template <int VEC>
__device__ __forceinline__ void row_load(const float* base, int64_t node, int64_t F,
                                         const Place& p, float (&v)[VEC]) {
  if (p.live) {
    load_vec<VEC>(base + node * F + p.foff, v);
  } else {
    zero<VEC>(v);
  }
}

// a lane's share of a dot product: one product, then fmas, in feature order
// (symmetric in its operands: the same bits whichever side was gathered)
template <int VEC>
__device__ __forceinline__ float lane_dot(const float (&x)[VEC], const float (&y)[VEC]) {
  float t = x[0] * y[0];
#pragma unroll
  for (int c = 1; c < VEC; ++c) t = __builtin_fmaf(x[c], y[c], t);
  return t;
}

// what a wave finds at its place in the schedule
enum Found { kPast, kSkip, kWalk };  // past the end | nothing to walk here | slots to walk

// the wave's (item of the schedule, head tile); false past the end
__device__ __forceinline__ bool wave_item(const Walk& a, int64_t items, int64_t& item,
                                          int64_t& tile) {
  const int64_t id = block_linear() * kWaves +
                     __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  item = id / a.tiles;
  tile = id - item * a.tiles;
  return item < items;
}

// the wave's row, item `it` of the schedule, of at most a chunk of slots
// (kSkip: a longer one, which is the pieces', or a row_order entry off the rows)
template <int64_t CHUNK>
__device__ __forceinline__ Found wave_row(const Walk& a, int64_t& it, int64_t& row, int64_t& tile,
                                          int64_t& beg, int64_t& end) {
  if (!wave_item(a, a.R, it, tile)) return kPast;
  row = a.row_order ? a.row_order[it] : it;
  row = __builtin_amdgcn_readfirstlane(static_cast<int>(row));
  if (row < 0 || row >= a.R) return kSkip;
  beg = clampi(a.indptr[row], 0, a.nnz);
  end = clampi(a.indptr[row + 1], beg, a.nnz);
  return (a.G > 0 && end - beg > CHUNK) ? kSkip : kWalk;
}

struct Piece {
  int64_t item, row, k0, k1, first, last;
};

// the wave's piece of a long row (kSkip: the item holds none)
template <int64_t CHUNK>
__device__ __forceinline__ Found wave_piece(const Walk& a, int lane, Piece& pc, int64_t& tile) {
  if (!wave_item(a, 2 * a.G, pc.item, tile)) return kPast;
  if (!long_row_piece(a.indptr, a.R, a.nnz, a.G, CHUNK, pc.item, lane, pc.row, pc.k0, pc.k1,
                      pc.first, pc.last))
    return kSkip;
  pc.row = uniform64(pc.row);
  pc.k0 = uniform64(pc.k0);
  pc.k1 = uniform64(pc.k1);
  pc.first = uniform64(pc.first);
  pc.last = uniform64(pc.last);
  return kWalk;
}

// ---------------------------------------------------------------------------
// the softmax
// ---------------------------------------------------------------------------
// One batch of the online softmax: s the batch's scores, summed over the head
// (and clamped or scaled by the caller), the first n of them slots, vv the
// slots' value rows. One rescale of (l, acc) to the new maximum, then the
// slots in slot order.
template <int BATCH, int VEC>
__device__ __forceinline__ void softmax_step(const float (&s)[BATCH], int n,
                                             const float (&vv)[BATCH][VEC], float& m, float& l,
                                             float (&acc)[VEC]) {
  float mn = m;
#pragma unroll
  for (int i = 0; i < BATCH; ++i) {
    if (i < n) mn = nanmax(mn, s[i]);
  }
  const float r = expf(m - mn);  // the first batch: expf(-inf) = 0 on zeros
  l = l * r;
#pragma unroll
  for (int c = 0; c < VEC; ++c) acc[c] = acc[c] * r;
#pragma unroll
  for (int i = 0; i < BATCH; ++i) {
    if (i < n) {
      const float e = expf(s[i] - mn);
      l = l + e;
#pragma unroll
      for (int c = 0; c < VEC; ++c) acc[c] = __builtin_fmaf(e, vv[i][c], acc[c]);
    }
  }
  m = mn;
}

// What follows reads a unit's own Args (the type A) by member name: o0 and
// stat, the outputs; ws0, ws1 and wsml, the pieces; dout, out and lse.

// out (a.o0) = acc / l and lse (a.stat) = m + logf(l) of a row; zeros for one
// without slots
template <int VEC, typename A>
__device__ __forceinline__ void fwd_store(const A& a, const Place& p, int64_t row, bool empty,
                                          float m, float l, const float (&acc)[VEC]) {
  float o[VEC];
#pragma unroll
  for (int c = 0; c < VEC; ++c) o[c] = empty ? 0.0f : acc[c] / l;
  if (p.live) store_vec<VEC>(a.o0 + row * a.H * a.D + p.foff, o);
  if (p.first) a.stat[row * a.H + p.head] = empty ? 0.0f : m + logf(l);
}

// The body of a forward's combine kernel: the wave of a long row's first piece
// merges the row's pieces (acc rows in a.ws0, (m, l) pairs in a.wsml, by item),
// in block order: the first one, then the items 2 g of the blocks up to the
// last.
template <int VEC, int64_t CHUNK, typename A>
__device__ __forceinline__ void fwd_combine(const A& a) {
  const int lane = threadIdx.x & 63;
  Piece pc;
  int64_t tile;
  if (wave_piece<CHUNK>(a, lane, pc, tile) != kWalk || pc.item != pc.first) return;
  const Place p = place_of<VEC>(a, tile, lane);
  const int64_t F = a.H * a.D;
  const float* ml = a.wsml + p.hsafe * 2;
  float m = ml[pc.first * a.H * 2];
  for (int64_t g = (pc.first >> 1) + 1; g <= pc.last; ++g) m = nanmax(m, ml[2 * g * a.H * 2]);
  float l = 0.0f, acc[VEC];
  zero<VEC>(acc);
  for (int64_t g = pc.first >> 1; g <= pc.last; ++g) {
    const int64_t item = g == (pc.first >> 1) ? pc.first : 2 * g;
    const float mg = ml[item * a.H * 2], lg = ml[item * a.H * 2 + 1];
    float pa[VEC];
    row_load<VEC>(a.ws0, item, F, p, pa);
    // a piece of only -inf beside a larger maximum adds nothing (its own sum
    // is NaN: -inf - -inf); when every piece is one, l stays 0 and out is NaN
    if (mg != -INFINITY) {
      const float w = expf(mg - m);
      l = __builtin_fmaf(lg, w, l);
#pragma unroll
      for (int c = 0; c < VEC; ++c) acc[c] = __builtin_fmaf(w, pa[c], acc[c]);
    }
  }
  fwd_store<VEC>(a, p, pc.row, false, m, l, acc);
}

// The body of a backward's sum-pieces kernel. The backward's pieces are
// partial sums: the wave of a long row's first piece adds them in block order
// into a.o0 (NOUT = 2: and a.o1 from the rows of a.ws1).
template <int VEC, int NOUT, int64_t CHUNK, typename A>
__device__ __forceinline__ void sum_pieces(const A& a) {
  const int lane = threadIdx.x & 63;
  Piece pc;
  int64_t tile;
  if (wave_piece<CHUNK>(a, lane, pc, tile) != kWalk || pc.item != pc.first) return;
  const Place p = place_of<VEC>(a, tile, lane);
  const int64_t F = a.H * a.D;
  float s0[VEC], s1[VEC], t[VEC];
  row_load<VEC>(a.ws0, pc.first, F, p, s0);
  if constexpr (NOUT == 2) row_load<VEC>(a.ws1, pc.first, F, p, s1);
  for (int64_t g = (pc.first >> 1) + 1; g <= pc.last; ++g) {
    row_load<VEC>(a.ws0, 2 * g, F, p, t);
#pragma unroll
    for (int c = 0; c < VEC; ++c) s0[c] = s0[c] + t[c];
    if constexpr (NOUT == 2) {
      row_load<VEC>(a.ws1, 2 * g, F, p, t);
#pragma unroll
      for (int c = 0; c < VEC; ++c) s1[c] = s1[c] + t[c];
    }
  }
  if (p.live) {
    store_vec<VEC>(a.o0 + pc.row * F + p.foff, s0);
    if constexpr (NOUT == 2) store_vec<VEC>(a.o1 + pc.row * F + p.foff, s1);
  }
}

// what a destination's wave holds of the backward: dout, lse and
// delta = <dout, out> of its head (a unit's DstRow adds its own row)
template <int VEC>
struct DstGrad {
  float dout[VEC];
  float lse, delta;
};

template <int VEC, typename A>
__device__ __forceinline__ void dst_grad(const A& a, const Place& p, int64_t row,
                                         DstGrad<VEC>& d) {
  const int64_t F = a.H * a.D;
  float ov[VEC], t[1];
  row_load<VEC>(a.dout, row, F, p, d.dout);
  row_load<VEC>(a.out, row, F, p, ov);
  d.lse = a.lse[row * a.H + p.hsafe];
  t[0] = lane_dot<VEC>(d.dout, ov);
  head_sum<1>(t, a.lph_shift);
  d.delta = t[0];
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
inline bool aligned(const void* p, uintptr_t n) {
  return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0;
}

inline int64_t num_blocks(int64_t nnz, int64_t chunk) { return (nnz + chunk - 1) / chunk; }

inline bool has_pieces(int64_t nnz, int64_t max_row_len, int64_t chunk) {
  return nnz > chunk && (max_row_len < 0 || max_row_len > chunk);
}

// the widest access every row of every tensor allows
inline int vec_of(int64_t D, std::initializer_list<const void*> ptrs) {
  int V = D % 4 == 0 ? 4 : (D % 2 == 0 ? 2 : 1);
  for (const void* p : ptrs) {
    while (V > 1 && p && !aligned(p, 4 * V)) V >>= 1;
  }
  return V;
}

// fills the lane map of `a` for VEC features a lane
inline void lane_map(Walk& a, int V) {
  const int64_t need = (a.D + V - 1) / V;
  DGLHIP_CHECK(need <= 64, "a head of " << a.D << " features is wider than the fused path's "
                                        << 64 * V << " at " << 4 * V << "-byte accesses");
  a.lph_shift = 0;
  while ((int64_t(1) << a.lph_shift) < need) ++a.lph_shift;
  const int64_t hpw = 64 >> a.lph_shift;
  a.tiles = (a.H + hpw - 1) / hpw;
}

inline dim3 waves_grid(int64_t waves) { return grid_1d((waves + kWaves - 1) / kWaves); }

inline void check_sizes(int64_t R, int64_t C, int64_t nnz, int64_t H, int64_t D) {
  DGLHIP_CHECK(R >= 0 && C >= 0 && nnz >= 0 && H >= 0 && D >= 0, "negative size");
  DGLHIP_CHECK(R < (int64_t(1) << 31) && C < (int64_t(1) << 31), "more than 2^31 - 1 nodes");
  DGLHIP_CHECK(nnz == 0 || C > 0, "slots without columns");
}

// f(std::integral_constant<int, V>()) for the V that vec_of found: the one
// place where the vector width turns into a template argument
template <typename Fn>
void with_vec(int V, Fn&& f) {
  if (V == 4) f(std::integral_constant<int, 4>());
  else if (V == 2) f(std::integral_constant<int, 2>());
  else f(std::integral_constant<int, 1>());
}

}  // namespace dglhip
