// Scaled dot-product attention over the edges of a graph, fused: for every
// destination r (a row of the CSR), head h and in-edge slot j with source u_j,
//
//   s_j = <q[r,h,:], k[u_j,h,:]> * scale, clamped to [lo, hi]
//   a_j = expf(s_j - max_j s_j) / sum_j expf(s_j - max_j s_j)
//   out[r,h,:] = sum_j a_j v[u_j,h,:],   lse[r,h] = max_j s_j + logf(sum_j ...)
//
// in one pass over the CSR, and its backward in two: dq over the same CSR,
// dk and dv over the transposed one, both recomputing s_j from q and k and
// a_j = expf(s_j - lse). Nothing of the size of the edge set is stored.
//
// Why no MFMA. Per edge the work is one gathered row of k against one row of
// q: a matrix-vector product whose matrix rows are scattered over memory and
// differ from destination to destination. A matrix instruction wants a tile
// of k shared by a tile of q rows; here two destinations share no sources, so
// a 4 x 4 or 32 x 32 tile would hold one useful row. The kernels are bound by
// the gathers, not by the 2 D flops per edge and head, and stay on the vector
// unit.
//
// Lane map, shared by the three kernels. A lane holds VEC consecutive
// features of one head (VEC = 4 with 16-byte accesses when D % 4 == 0 and
// every tensor is 16-byte aligned, else 2 with 8-byte ones, else 1). A head
// takes LPH lanes, the power of two that covers D / VEC (lanes past D idle,
// they hold zeros), a wave covers 64 / LPH heads, and more heads than that
// are further head tiles: a wave is one (row, head tile), since a head's
// softmax is its own. A dot product is summed per lane over its VEC features
// (one product, then fmas, in feature order) and then across the head's
// lanes by an xor butterfly: DPP at strides 1, 2 (quad permutes), 4, 8 (the
// mirrors of 8 and 16 lanes: after the earlier stages a mirror's partner
// holds what the xor partner holds), __shfl_xor at 16 and 32. Both partners
// of a stage add the same two numbers, so every lane of a head ends with the
// same bits, and the three kernels compute the same bits for s_j: the clamp
// is active in all of them or in none.
//
// The walk. A wave takes up to 64 column ids of its row in one coalesced load
// and hands them out lane to lane; it runs the slots in batches of
// DGLHIP_DOT_ATTENTION_BATCH: the batch's gathers (2 rows per slot) are issued
// before first use, then the dots, then, in the forward, one rescale
// expf(m - m') of the running sum and the VEC accumulators per batch (m' the
// maximum of m and the batch's scores) and per slot, in slot order,
// p = expf(s - m'), l += p, acc = fma(p, v, acc).
//
// Long rows. A row of more than DGLHIP_DOT_ATTENTION_CHUNK slots is cut where
// it crosses the multiples of the chunk (row_pieces.h), a piece a wave. In
// the forward a piece leaves (m, l, acc[D]) per head in the workspace and the
// wave of the row's first piece merges them in block order (m = max m_g,
// weights expf(m_g - m)) and stores out and lse; in the backward lse and
// delta are known, the pieces are plain partial sums, added in block order.
//
// No atomics; every output element has one writer: the same bits on every call.
#include "../../include/dgl_hip.h"
#include "attention_lanes.h"
#include "common.h"
#include "launch.h"
#include "row_pieces.h"

#include <hip/hip_runtime.h>

#include <cmath>

namespace dglhip {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int64_t kChunk = DGLHIP_DOT_ATTENTION_CHUNK;
constexpr int kBatch = DGLHIP_DOT_ATTENTION_BATCH;

// (a NaN passes through, as through torch.clamp)
__device__ __forceinline__ float clamp_score(float s, float lo, float hi) {
  return s < lo ? lo : (s > hi ? hi : s);
}

struct Args {
  int64_t R, C, nnz, H, D;  // rows and columns of the CSR the kernel walks
  int64_t G;                // blocks of kChunk slots (0: no row is longer than a chunk)
  int64_t tiles;            // head tiles per row
  int lph_shift;            // log2 of the lanes per head
  float scale, lo, hi;
  const int64_t* indptr;
  const int32_t* indices;
  const int32_t* row_order;
  const float *q, *k, *v;       // q by destination, k and v by source
  const float *dout, *out;      // by destination (backward)
  const float *lse, *delta;     // (destinations, H), read (backward)
  float *o0, *o1;               // out | dq | dk, dv
  float* stat;                  // lse (forward) or delta (dq), written
  float *ws0, *ws1, *wsml;      // the pieces: 2 G rows of H D floats twice, 2 G H (m, l) pairs
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
__device__ __forceinline__ Place place_of(const Args& a, int64_t tile, int lane) {
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
__device__ __forceinline__ void row_load(const float* base, int64_t node, int64_t F,
                                         const Place& p, float (&v)[VEC]) {
  if (p.live) {
    load_vec<VEC>(base + node * F + p.foff, v);
  } else {
#pragma unroll
    for (int c = 0; c < VEC; ++c) v[c] = 0.0f;
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

// the slots [k0, k1) in batches of kBatch column ids (attention_lanes.h)
template <typename Body>
__device__ __forceinline__ void for_batches(const Args& a, int64_t k0, int64_t k1, int lane,
                                            Body&& body) {
  batch_ids<kBatch>(a.indices, a.C, k0, k1, lane, body);
}

// the wave's (item of the schedule, head tile); false past the end
__device__ __forceinline__ bool wave_item(const Args& a, int64_t items, int64_t& item,
                                          int64_t& tile) {
  const int64_t id = block_linear() * kWaves +
                     __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  item = id / a.tiles;
  tile = id - item * a.tiles;
  return item < items;
}

// the wave's row of at most a chunk of slots (longer ones are the pieces')
__device__ __forceinline__ bool wave_row(const Args& a, int64_t& row, int64_t& tile, int64_t& beg,
                                         int64_t& end) {
  int64_t it;
  if (!wave_item(a, a.R, it, tile)) return false;
  row = a.row_order ? a.row_order[it] : it;
  row = __builtin_amdgcn_readfirstlane(static_cast<int>(row));
  if (row < 0 || row >= a.R) return false;
  beg = clampi(a.indptr[row], 0, a.nnz);
  end = clampi(a.indptr[row + 1], beg, a.nnz);
  return !(a.G > 0 && end - beg > kChunk);
}

struct Piece {
  int64_t item, row, k0, k1, first, last;
};

// the wave's piece of a long row
__device__ __forceinline__ bool wave_piece(const Args& a, int lane, Piece& pc, int64_t& tile) {
  if (!wave_item(a, 2 * a.G, pc.item, tile)) return false;
  if (!long_row_piece(a.indptr, a.R, a.nnz, a.G, kChunk, pc.item, lane, pc.row, pc.k0, pc.k1,
                      pc.first, pc.last))
    return false;
  pc.row = uniform64(pc.row);
  pc.k0 = uniform64(pc.k0);
  pc.k1 = uniform64(pc.k1);
  pc.first = uniform64(pc.first);
  pc.last = uniform64(pc.last);
  return true;
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <int VEC>
__device__ __forceinline__ void fwd_range(const Args& a, const Place& p, int lane,
                                          const float (&qv)[VEC], int64_t k0, int64_t k1,
                                          float& m, float& l, float (&acc)[VEC]) {
  const int64_t F = a.H * a.D;
  for_batches(a, k0, k1, lane, [&](const int (&u)[kBatch], int n) {
    float kk[kBatch][VEC], vv[kBatch][VEC], s[kBatch];
#pragma unroll
    for (int i = 0; i < kBatch; ++i) row_load<VEC>(a.k, u[i], F, p, kk[i]);
#pragma unroll
    for (int i = 0; i < kBatch; ++i) row_load<VEC>(a.v, u[i], F, p, vv[i]);
#pragma unroll
    for (int i = 0; i < kBatch; ++i) s[i] = lane_dot<VEC>(qv, kk[i]);
    head_sum<kBatch>(s, a.lph_shift);
    float mn = m;
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      s[i] = clamp_score(s[i] * a.scale, a.lo, a.hi);
      if (i < n) mn = nanmax(mn, s[i]);
    }
    const float r = expf(m - mn);  // the first batch: expf(-inf) = 0 on zeros
    l = l * r;
#pragma unroll
    for (int c = 0; c < VEC; ++c) acc[c] = acc[c] * r;
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      if (i < n) {
        const float e = expf(s[i] - mn);
        l = l + e;
#pragma unroll
        for (int c = 0; c < VEC; ++c) acc[c] = __builtin_fmaf(e, vv[i][c], acc[c]);
      }
    }
    m = mn;
  });
}

template <int VEC>
__device__ __forceinline__ void fwd_store(const Args& a, const Place& p, int64_t row, bool empty,
                                          float m, float l, const float (&acc)[VEC]) {
  float o[VEC];
#pragma unroll
  for (int c = 0; c < VEC; ++c) o[c] = empty ? 0.0f : acc[c] / l;
  if (p.live) store_vec<VEC>(a.o0 + row * a.H * a.D + p.foff, o);
  if (p.first) a.stat[row * a.H + p.head] = empty ? 0.0f : m + logf(l);
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void dot_attention_fwd_rows_kernel(Args a) {
  const int lane = threadIdx.x & 63;
  int64_t row, tile, beg, end;
  if (!wave_row(a, row, tile, beg, end)) return;  // the whole wave
  const Place p = place_of<VEC>(a, tile, lane);
  float qv[VEC], acc[VEC];
  row_load<VEC>(a.q, row, a.H * a.D, p, qv);
  float m = -INFINITY, l = 0.0f;
#pragma unroll
  for (int c = 0; c < VEC; ++c) acc[c] = 0.0f;
  fwd_range<VEC>(a, p, lane, qv, beg, end, m, l, acc);
  fwd_store<VEC>(a, p, row, beg == end, m, l, acc);
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void dot_attention_fwd_piece_kernel(Args a) {
  const int lane = threadIdx.x & 63;
  Piece pc;
  int64_t tile;
  if (!wave_piece(a, lane, pc, tile)) return;  // the whole wave
  const Place p = place_of<VEC>(a, tile, lane);
  float qv[VEC], acc[VEC];
  row_load<VEC>(a.q, pc.row, a.H * a.D, p, qv);
  float m = -INFINITY, l = 0.0f;
#pragma unroll
  for (int c = 0; c < VEC; ++c) acc[c] = 0.0f;
  fwd_range<VEC>(a, p, lane, qv, pc.k0, pc.k1, m, l, acc);
  if (p.live) store_vec<VEC>(a.ws0 + pc.item * a.H * a.D + p.foff, acc);
  if (p.first) {
    a.wsml[(pc.item * a.H + p.head) * 2] = m;
    a.wsml[(pc.item * a.H + p.head) * 2 + 1] = l;
  }
}

// The wave of a long row's first piece merges the row's pieces, in block
// order: the first one, then the items 2 g of the blocks up to the last.
template <int VEC>
__global__ __launch_bounds__(kThreads) void dot_attention_fwd_combine_kernel(Args a) {
  const int lane = threadIdx.x & 63;
  Piece pc;
  int64_t tile;
  if (!wave_piece(a, lane, pc, tile) || pc.item != pc.first) return;
  const Place p = place_of<VEC>(a, tile, lane);
  const int64_t F = a.H * a.D;
  const float* ml = a.wsml + p.hsafe * 2;
  float m = ml[pc.first * a.H * 2];
  for (int64_t g = (pc.first >> 1) + 1; g <= pc.last; ++g) m = nanmax(m, ml[2 * g * a.H * 2]);
  float l = 0.0f, acc[VEC];
#pragma unroll
  for (int c = 0; c < VEC; ++c) acc[c] = 0.0f;
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

// ---------------------------------------------------------------------------
// backward over the forward CSR: delta and dq
// ---------------------------------------------------------------------------
// The gradient of a clamped score is torch.clamp's: 0 strictly outside
// [lo, hi], the incoming gradient on the bounds and inside.
__device__ __forceinline__ float score_grad(const Args& a, float raw, float lse, float dp,
                                            float delta, float& e) {
  e = expf(clamp_score(raw, a.lo, a.hi) - lse);
  const float ds = e * (dp - delta);
  return (raw < a.lo || raw > a.hi) ? 0.0f : ds * a.scale;
}

// what a destination's wave holds: q, dout, lse and delta = <dout, out> of its head
template <int VEC>
struct DstRow {
  float q[VEC], dout[VEC];
  float lse, delta;
};

template <int VEC>
__device__ __forceinline__ DstRow<VEC> dst_row(const Args& a, const Place& p, int64_t row) {
  DstRow<VEC> d;
  const int64_t F = a.H * a.D;
  float ov[VEC], t[1];
  row_load<VEC>(a.q, row, F, p, d.q);
  row_load<VEC>(a.dout, row, F, p, d.dout);
  row_load<VEC>(a.out, row, F, p, ov);
  d.lse = a.lse[row * a.H + p.hsafe];
  t[0] = lane_dot<VEC>(d.dout, ov);
  head_sum<1>(t, a.lph_shift);
  d.delta = t[0];
  return d;
}

template <int VEC>
__device__ __forceinline__ void dq_range(const Args& a, const Place& p, int lane,
                                         const DstRow<VEC>& d, int64_t k0, int64_t k1,
                                         float (&dq)[VEC]) {
  const int64_t F = a.H * a.D;
  for_batches(a, k0, k1, lane, [&](const int (&u)[kBatch], int n) {
    float kk[kBatch][VEC], vv[kBatch][VEC], s[kBatch], dp[kBatch];
#pragma unroll
    for (int i = 0; i < kBatch; ++i) row_load<VEC>(a.k, u[i], F, p, kk[i]);
#pragma unroll
    for (int i = 0; i < kBatch; ++i) row_load<VEC>(a.v, u[i], F, p, vv[i]);
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      s[i] = lane_dot<VEC>(d.q, kk[i]);
      dp[i] = lane_dot<VEC>(d.dout, vv[i]);
    }
    head_sum<kBatch>(s, a.lph_shift);
    head_sum<kBatch>(dp, a.lph_shift);
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      if (i < n) {
        float e;
        const float t = score_grad(a, s[i] * a.scale, d.lse, dp[i], d.delta, e);
#pragma unroll
        for (int c = 0; c < VEC; ++c) dq[c] = __builtin_fmaf(t, kk[i][c], dq[c]);
      }
    }
  });
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void dot_attention_dq_rows_kernel(Args a) {
  const int lane = threadIdx.x & 63;
  int64_t row, tile, beg, end;
  if (!wave_row(a, row, tile, beg, end)) return;  // the whole wave
  const Place p = place_of<VEC>(a, tile, lane);
  const DstRow<VEC> d = dst_row<VEC>(a, p, row);
  if (p.first) a.stat[row * a.H + p.head] = d.delta;
  float dq[VEC];
#pragma unroll
  for (int c = 0; c < VEC; ++c) dq[c] = 0.0f;
  dq_range<VEC>(a, p, lane, d, beg, end, dq);
  if (p.live) store_vec<VEC>(a.o0 + row * a.H * a.D + p.foff, dq);
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void dot_attention_dq_piece_kernel(Args a) {
  const int lane = threadIdx.x & 63;
  Piece pc;
  int64_t tile;
  if (!wave_piece(a, lane, pc, tile)) return;  // the whole wave
  const Place p = place_of<VEC>(a, tile, lane);
  const DstRow<VEC> d = dst_row<VEC>(a, p, pc.row);
  if (p.first && pc.item == pc.first) a.stat[pc.row * a.H + p.head] = d.delta;
  float dq[VEC];
#pragma unroll
  for (int c = 0; c < VEC; ++c) dq[c] = 0.0f;
  dq_range<VEC>(a, p, lane, d, pc.k0, pc.k1, dq);
  if (p.live) store_vec<VEC>(a.ws0 + pc.item * a.H * a.D + p.foff, dq);
}

// The backward's pieces are partial sums: the wave of a long row's first
// piece adds them in block order (NOUT = 2: dk from ws0 and dv from ws1).
template <int VEC, int NOUT>
__global__ __launch_bounds__(kThreads) void dot_attention_sum_pieces_kernel(Args a) {
  const int lane = threadIdx.x & 63;
  Piece pc;
  int64_t tile;
  if (!wave_piece(a, lane, pc, tile) || pc.item != pc.first) return;
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

// ---------------------------------------------------------------------------
// backward over the transposed CSR: dk and dv, a wave per (source, head tile)
// ---------------------------------------------------------------------------
template <int VEC>
__device__ __forceinline__ void dkv_range(const Args& a, const Place& p, int lane,
                                          const float (&kv)[VEC], const float (&vv)[VEC],
                                          int64_t k0, int64_t k1, float (&dk)[VEC],
                                          float (&dv)[VEC]) {
  const int64_t F = a.H * a.D;
  for_batches(a, k0, k1, lane, [&](const int (&r)[kBatch], int n) {
    float qq[kBatch][VEC], dd[kBatch][VEC], ls[kBatch], de[kBatch], s[kBatch], dp[kBatch];
#pragma unroll
    for (int i = 0; i < kBatch; ++i) row_load<VEC>(a.q, r[i], F, p, qq[i]);
#pragma unroll
    for (int i = 0; i < kBatch; ++i) row_load<VEC>(a.dout, r[i], F, p, dd[i]);
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      // (one 4-byte load for the lanes of a head)
      ls[i] = a.lse[r[i] * a.H + p.hsafe];
      de[i] = a.delta[r[i] * a.H + p.hsafe];
    }
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      s[i] = lane_dot<VEC>(qq[i], kv);
      dp[i] = lane_dot<VEC>(dd[i], vv);
    }
    head_sum<kBatch>(s, a.lph_shift);
    head_sum<kBatch>(dp, a.lph_shift);
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      if (i < n) {
        float e;
        const float t = score_grad(a, s[i] * a.scale, ls[i], dp[i], de[i], e);
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
          dv[c] = __builtin_fmaf(e, dd[i][c], dv[c]);
          dk[c] = __builtin_fmaf(t, qq[i][c], dk[c]);
        }
      }
    }
  });
}

template <int VEC, bool PIECE>
__global__ __launch_bounds__(kThreads) void dot_attention_dkv_kernel(Args a) {
  const int lane = threadIdx.x & 63;
  int64_t row, tile, beg, end, at;
  if constexpr (PIECE) {
    Piece pc;
    if (!wave_piece(a, lane, pc, tile)) return;  // the whole wave
    row = pc.row; beg = pc.k0; end = pc.k1; at = pc.item;
  } else {
    if (!wave_row(a, row, tile, beg, end)) return;
    at = row;
  }
  const Place p = place_of<VEC>(a, tile, lane);
  const int64_t F = a.H * a.D;
  float kv[VEC], vv[VEC], dk[VEC], dv[VEC];
  row_load<VEC>(a.k, row, F, p, kv);
  row_load<VEC>(a.v, row, F, p, vv);
#pragma unroll
  for (int c = 0; c < VEC; ++c) dk[c] = dv[c] = 0.0f;
  dkv_range<VEC>(a, p, lane, kv, vv, beg, end, dk, dv);
  if (p.live) {
    store_vec<VEC>((PIECE ? a.ws0 : a.o0) + at * F + p.foff, dk);
    store_vec<VEC>((PIECE ? a.ws1 : a.o1) + at * F + p.foff, dv);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
bool aligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

int64_t num_blocks(int64_t nnz) { return (nnz + kChunk - 1) / kChunk; }

bool has_pieces(int64_t nnz, int64_t max_row_len) {
  return nnz > kChunk && (max_row_len < 0 || max_row_len > kChunk);
}

// the widest access every row of every tensor allows
int vec_of(int64_t D, std::initializer_list<const void*> ptrs) {
  int V = D % 4 == 0 ? 4 : (D % 2 == 0 ? 2 : 1);
  for (const void* p : ptrs) {
    while (V > 1 && p && !aligned(p, 4 * V)) V >>= 1;
  }
  return V;
}

// fills the lane map of `a` for VEC features a lane
void lane_map(Args& a, int V) {
  const int64_t need = (a.D + V - 1) / V;
  DGLHIP_CHECK(need <= 64, "a head of " << a.D << " features is wider than the fused path's "
                                        << 64 * V << " at " << 4 * V << "-byte accesses");
  a.lph_shift = 0;
  while ((int64_t(1) << a.lph_shift) < need) ++a.lph_shift;
  const int64_t hpw = 64 >> a.lph_shift;
  a.tiles = (a.H + hpw - 1) / hpw;
}

void pieces_of(Args& a, int64_t max_row_len, void* workspace) {
  const bool pieces = has_pieces(a.nnz, max_row_len);
  DGLHIP_CHECK(!pieces || workspace, "rows longer than a chunk need the workspace");
  a.G = pieces ? num_blocks(a.nnz) : 0;
  float* ws = static_cast<float*>(workspace);
  a.ws0 = ws;
  a.ws1 = ws + 2 * a.G * a.H * a.D;
  a.wsml = ws + 4 * a.G * a.H * a.D;
}

dim3 waves_grid(int64_t waves) { return grid_1d((waves + kWaves - 1) / kWaves); }

#define DOT_ATTENTION_LAUNCH(V, grid, stream, a, ...)                                   \
  do {                                                                                  \
    if ((V) == 4)                                                                       \
      hipLaunchKernelGGL((__VA_ARGS__<4>), grid, dim3(kThreads), 0, stream, a);         \
    else if ((V) == 2)                                                                  \
      hipLaunchKernelGGL((__VA_ARGS__<2>), grid, dim3(kThreads), 0, stream, a);         \
    else                                                                                \
      hipLaunchKernelGGL((__VA_ARGS__<1>), grid, dim3(kThreads), 0, stream, a);         \
  } while (0)

template <int V, int NOUT>
void launch_sum_pieces(dim3 grid, hipStream_t stream, const Args& a) {
  hipLaunchKernelGGL((dot_attention_sum_pieces_kernel<V, NOUT>), grid, dim3(kThreads), 0, stream,
                     a);
}

template <int V, bool PIECE>
void launch_dkv(dim3 grid, hipStream_t stream, const Args& a) {
  hipLaunchKernelGGL((dot_attention_dkv_kernel<V, PIECE>), grid, dim3(kThreads), 0, stream, a);
}

template <int V>
void backward_v(const Args& aq, const Args& at, hipStream_t stream) {
  if (aq.R > 0)
    hipLaunchKernelGGL((dot_attention_dq_rows_kernel<V>), waves_grid(aq.R * aq.tiles),
                       dim3(kThreads), 0, stream, aq);
  if (aq.G > 0) {
    const dim3 pgrid = waves_grid(2 * aq.G * aq.tiles);
    hipLaunchKernelGGL((dot_attention_dq_piece_kernel<V>), pgrid, dim3(kThreads), 0, stream, aq);
    launch_sum_pieces<V, 1>(pgrid, stream, aq);
  }
  DGLHIP_CHECK(hipGetLastError() == hipSuccess, "dot attention dq launch failed");
  if (at.R == 0) return;
  // (after dq on the stream: both halves' pieces go through one workspace)
  launch_dkv<V, false>(waves_grid(at.R * at.tiles), stream, at);
  if (at.G > 0) {
    const dim3 pgrid = waves_grid(2 * at.G * at.tiles);
    launch_dkv<V, true>(pgrid, stream, at);
    launch_sum_pieces<V, 2>(pgrid, stream, at);
  }
  DGLHIP_CHECK(hipGetLastError() == hipSuccess, "dot attention dk / dv launch failed");
}

void check_sizes(int64_t R, int64_t C, int64_t nnz, int64_t H, int64_t D) {
  DGLHIP_CHECK(R >= 0 && C >= 0 && nnz >= 0 && H >= 0 && D >= 0, "negative size");
  DGLHIP_CHECK(R < (int64_t(1) << 31) && C < (int64_t(1) << 31), "more than 2^31 - 1 nodes");
  DGLHIP_CHECK(nnz == 0 || C > 0, "slots without columns");
}

}  // namespace

}  // namespace dglhip

using namespace dglhip;

extern "C" {

int64_t dglhip_dot_attention_workspace_bytes(int64_t num_rows, int64_t nnz, int64_t num_heads,
                                             int64_t head_dim, int64_t max_row_len) {
  if (num_rows <= 0 || num_heads <= 0 || head_dim <= 0 || !has_pieces(nnz, max_row_len)) return 0;
  return 2 * num_blocks(nnz) * (2 * num_heads * head_dim + 2 * num_heads) * 4;
}

int dglhip_dot_attention_device(int64_t num_rows, int64_t num_cols, int64_t nnz,
                                int64_t num_heads, int64_t head_dim, const int64_t* indptr,
                                const int32_t* indices, const int32_t* row_order, const float* q,
                                const float* k, const float* v, float scale, float lo, float hi,
                                float* out, float* lse, int64_t max_row_len, void* workspace,
                                void* stream) {
  API_BEGIN();
  check_sizes(num_rows, num_cols, nnz, num_heads, head_dim);
  if (num_rows == 0 || num_heads == 0 || head_dim == 0) return 0;
  DGLHIP_CHECK(indptr && q && out && lse && (nnz == 0 || (indices && k && v)),
               "null pointer argument");
  Args a = {};
  a.R = num_rows; a.C = num_cols; a.nnz = nnz; a.H = num_heads; a.D = head_dim;
  a.scale = scale; a.lo = lo; a.hi = hi;
  a.indptr = indptr; a.indices = indices; a.row_order = row_order;
  a.q = q; a.k = k; a.v = v;
  a.o0 = out; a.stat = lse;
  pieces_of(a, max_row_len, workspace);
  const int V = vec_of(head_dim, {q, k, v, out, a.G ? workspace : nullptr});
  lane_map(a, V);
  hipStream_t st = static_cast<hipStream_t>(stream);
  DOT_ATTENTION_LAUNCH(V, waves_grid(a.R * a.tiles), st, a, dot_attention_fwd_rows_kernel);
  if (a.G > 0) {
    const dim3 pgrid = waves_grid(2 * a.G * a.tiles);
    DOT_ATTENTION_LAUNCH(V, pgrid, st, a, dot_attention_fwd_piece_kernel);
    DOT_ATTENTION_LAUNCH(V, pgrid, st, a, dot_attention_fwd_combine_kernel);
  }
  DGLHIP_CHECK(hipGetLastError() == hipSuccess, "dot attention launch failed");
  API_END();
}

int dglhip_dot_attention_bwd_device(int64_t num_rows, int64_t num_cols, int64_t nnz,
                                    int64_t num_heads, int64_t head_dim, const int64_t* indptr,
                                    const int32_t* indices, const int32_t* row_order,
                                    const int64_t* t_indptr, const int32_t* t_indices,
                                    const int32_t* t_row_order, const float* q, const float* k,
                                    const float* v, const float* out, const float* lse,
                                    const float* dout, float scale, float lo, float hi,
                                    float* delta, float* dq, float* dk, float* dv,
                                    int64_t max_row_len, int64_t max_col_len, void* workspace,
                                    void* stream) {
  API_BEGIN();
  check_sizes(num_rows, num_cols, nnz, num_heads, head_dim);
  if (num_heads == 0 || head_dim == 0 || (num_rows == 0 && num_cols == 0)) return 0;
  DGLHIP_CHECK(indptr && t_indptr && q && k && v && out && lse && dout && delta && dq && dk && dv &&
                   (nnz == 0 || (indices && t_indices)),
               "null pointer argument");
  Args aq = {};
  aq.R = num_rows; aq.C = num_cols; aq.nnz = nnz; aq.H = num_heads; aq.D = head_dim;
  aq.scale = scale; aq.lo = lo; aq.hi = hi;
  aq.indptr = indptr; aq.indices = indices; aq.row_order = row_order;
  aq.q = q; aq.k = k; aq.v = v; aq.dout = dout; aq.out = out; aq.lse = lse;
  aq.o0 = dq; aq.stat = delta;
  pieces_of(aq, max_row_len, workspace);
  Args at = aq;
  at.R = num_cols; at.C = num_rows;
  at.indptr = t_indptr; at.indices = t_indices; at.row_order = t_row_order;
  at.delta = delta; at.o0 = dk; at.o1 = dv; at.stat = nullptr;
  pieces_of(at, max_col_len, workspace);
  const int V = vec_of(head_dim, {q, k, v, out, dout, dq, dk, dv,
                                  (aq.G || at.G) ? workspace : nullptr});
  lane_map(aq, V);
  lane_map(at, V);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (V == 4) backward_v<4>(aq, at, st);
  else if (V == 2) backward_v<2>(aq, at, st);
  else backward_v<1>(aq, at, st);
  API_END();
}

}  // extern "C"
