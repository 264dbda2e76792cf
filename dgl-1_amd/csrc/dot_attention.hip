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
// The lane map, the walk in batches, the online softmax and the pieces of long
// rows are attention_walk.h's, shared with gatv2_attention.hip. Here: the batch
// is DGLHIP_DOT_ATTENTION_BATCH slots of 2 gathered rows each (k and v), the
// chunk DGLHIP_DOT_ATTENTION_CHUNK, and the three walks compute the same bits
// for s_j, so the clamp is active in all of them or in none.
//
// No atomics; every output element has one writer: the same bits on every call.
#include "../../include/dgl_hip.h"
#include "attention_walk.h"

#include <hip/hip_runtime.h>

#include <cmath>

namespace dglhip {

namespace {

constexpr int64_t kChunk = DGLHIP_DOT_ATTENTION_CHUNK;
constexpr int kBatch = DGLHIP_DOT_ATTENTION_BATCH;

// (a NaN passes through, as through torch.clamp)
__device__ __forceinline__ float clamp_score(float s, float lo, float hi) {
  return s < lo ? lo : (s > hi ? hi : s);
}

struct Args : Walk {
  float scale, lo, hi;
  const float *q, *k, *v;       // q by destination, k and v by source
  const float *dout, *out;      // by destination (backward)
  const float *lse, *delta;     // (destinations, H), read (backward)
  float *o0, *o1;               // out | dq | dk, dv
  float* stat;                  // lse (forward) or delta (dq), written
  float *ws0, *ws1, *wsml;      // the pieces: 2 G rows of H D floats twice, 2 G H (m, l) pairs
};

// the slots [k0, k1) in batches of kBatch column ids (attention_lanes.h)
template <typename Body>
__device__ __forceinline__ void for_batches(const Args& a, int64_t k0, int64_t k1, int lane,
                                            Body&& body) {
  batch_ids<kBatch>(a.indices, a.C, k0, k1, lane, body);
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
#pragma unroll
    for (int i = 0; i < kBatch; ++i) s[i] = clamp_score(s[i] * a.scale, a.lo, a.hi);
    softmax_step<kBatch, VEC>(s, n, vv, m, l, acc);
  });
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void dot_attention_fwd_rows_kernel(Args a) {
  const int lane = threadIdx.x & 63;
  int64_t it, row, tile, beg, end;
  if (wave_row<kChunk>(a, it, row, tile, beg, end) != kWalk) return;  // the whole wave
  const Place p = place_of<VEC>(a, tile, lane);
  float qv[VEC], acc[VEC];
  row_load<VEC>(a.q, row, a.H * a.D, p, qv);
  float m = -INFINITY, l = 0.0f;
  zero<VEC>(acc);
  fwd_range<VEC>(a, p, lane, qv, beg, end, m, l, acc);
  fwd_store<VEC>(a, p, row, beg == end, m, l, acc);
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void dot_attention_fwd_piece_kernel(Args a) {
  const int lane = threadIdx.x & 63;
  Piece pc;
  int64_t tile;
  if (wave_piece<kChunk>(a, lane, pc, tile) != kWalk) return;  // the whole wave
  const Place p = place_of<VEC>(a, tile, lane);
  float qv[VEC], acc[VEC];
  row_load<VEC>(a.q, pc.row, a.H * a.D, p, qv);
  float m = -INFINITY, l = 0.0f;
  zero<VEC>(acc);
  fwd_range<VEC>(a, p, lane, qv, pc.k0, pc.k1, m, l, acc);
  if (p.live) store_vec<VEC>(a.ws0 + pc.item * a.H * a.D + p.foff, acc);
  if (p.first) {
    a.wsml[(pc.item * a.H + p.head) * 2] = m;
    a.wsml[(pc.item * a.H + p.head) * 2 + 1] = l;
  }
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void dot_attention_fwd_combine_kernel(Args a) {
  fwd_combine<VEC, kChunk>(a);
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

// what a destination's wave holds: q, and dout, lse and delta of its head
template <int VEC>
struct DstRow : DstGrad<VEC> {
  float q[VEC];
};

template <int VEC>
__device__ __forceinline__ DstRow<VEC> dst_row(const Args& a, const Place& p, int64_t row) {
  DstRow<VEC> d;
  row_load<VEC>(a.q, row, a.H * a.D, p, d.q);
  dst_grad<VEC>(a, p, row, d);
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
  int64_t it, row, tile, beg, end;
  if (wave_row<kChunk>(a, it, row, tile, beg, end) != kWalk) return;  // the whole wave
  const Place p = place_of<VEC>(a, tile, lane);
  const DstRow<VEC> d = dst_row<VEC>(a, p, row);
  if (p.first) a.stat[row * a.H + p.head] = d.delta;
  float dq[VEC];
  zero<VEC>(dq);
  dq_range<VEC>(a, p, lane, d, beg, end, dq);
  if (p.live) store_vec<VEC>(a.o0 + row * a.H * a.D + p.foff, dq);
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void dot_attention_dq_piece_kernel(Args a) {
  const int lane = threadIdx.x & 63;
  Piece pc;
  int64_t tile;
  if (wave_piece<kChunk>(a, lane, pc, tile) != kWalk) return;  // the whole wave
  const Place p = place_of<VEC>(a, tile, lane);
  const DstRow<VEC> d = dst_row<VEC>(a, p, pc.row);
  if (p.first && pc.item == pc.first) a.stat[pc.row * a.H + p.head] = d.delta;
  float dq[VEC];
  zero<VEC>(dq);
  dq_range<VEC>(a, p, lane, d, pc.k0, pc.k1, dq);
  if (p.live) store_vec<VEC>(a.ws0 + pc.item * a.H * a.D + p.foff, dq);
}

// (NOUT = 2: dk from ws0 and dv from ws1)
template <int VEC, int NOUT>
__global__ __launch_bounds__(kThreads) void dot_attention_sum_pieces_kernel(Args a) {
  sum_pieces<VEC, NOUT, kChunk>(a);
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
    if (wave_piece<kChunk>(a, lane, pc, tile) != kWalk) return;  // the whole wave
    row = pc.row; beg = pc.k0; end = pc.k1; at = pc.item;
  } else {
    int64_t it;
    if (wave_row<kChunk>(a, it, row, tile, beg, end) != kWalk) return;
    at = row;
  }
  const Place p = place_of<VEC>(a, tile, lane);
  const int64_t F = a.H * a.D;
  float kv[VEC], vv[VEC], dk[VEC], dv[VEC];
  row_load<VEC>(a.k, row, F, p, kv);
  row_load<VEC>(a.v, row, F, p, vv);
  zero<VEC>(dk);
  zero<VEC>(dv);
  dkv_range<VEC>(a, p, lane, kv, vv, beg, end, dk, dv);
  if (p.live) {
    store_vec<VEC>((PIECE ? a.ws0 : a.o0) + at * F + p.foff, dk);
    store_vec<VEC>((PIECE ? a.ws1 : a.o1) + at * F + p.foff, dv);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
void pieces_of(Args& a, int64_t max_row_len, void* workspace) {
  const bool pieces = has_pieces(a.nnz, max_row_len, kChunk);
  DGLHIP_CHECK(!pieces || workspace, "rows longer than a chunk need the workspace");
  a.G = pieces ? num_blocks(a.nnz, kChunk) : 0;
  float* ws = static_cast<float*>(workspace);
  a.ws0 = ws;
  a.ws1 = ws + 2 * a.G * a.H * a.D;
  a.wsml = ws + 4 * a.G * a.H * a.D;
}

template <int V>
void forward_v(const Args& a, hipStream_t stream) {
  hipLaunchKernelGGL((dot_attention_fwd_rows_kernel<V>), waves_grid(a.R * a.tiles), dim3(kThreads),
                     0, stream, a);
  if (a.G > 0) {
    const dim3 pgrid = waves_grid(2 * a.G * a.tiles);
    hipLaunchKernelGGL((dot_attention_fwd_piece_kernel<V>), pgrid, dim3(kThreads), 0, stream, a);
    hipLaunchKernelGGL((dot_attention_fwd_combine_kernel<V>), pgrid, dim3(kThreads), 0, stream, a);
  }
  DGLHIP_CHECK(hipGetLastError() == hipSuccess, "dot attention launch failed");
}

template <int V>
void backward_v(const Args& aq, const Args& at, hipStream_t stream) {
  if (aq.R > 0)
    hipLaunchKernelGGL((dot_attention_dq_rows_kernel<V>), waves_grid(aq.R * aq.tiles),
                       dim3(kThreads), 0, stream, aq);
  if (aq.G > 0) {
    const dim3 pgrid = waves_grid(2 * aq.G * aq.tiles);
    hipLaunchKernelGGL((dot_attention_dq_piece_kernel<V>), pgrid, dim3(kThreads), 0, stream, aq);
    hipLaunchKernelGGL((dot_attention_sum_pieces_kernel<V, 1>), pgrid, dim3(kThreads), 0, stream,
                       aq);
  }
  DGLHIP_CHECK(hipGetLastError() == hipSuccess, "dot attention dq launch failed");
  if (at.R == 0) return;
  // (after dq on the stream: both halves' pieces go through one workspace)
  hipLaunchKernelGGL((dot_attention_dkv_kernel<V, false>), waves_grid(at.R * at.tiles),
                     dim3(kThreads), 0, stream, at);
  if (at.G > 0) {
    const dim3 pgrid = waves_grid(2 * at.G * at.tiles);
    hipLaunchKernelGGL((dot_attention_dkv_kernel<V, true>), pgrid, dim3(kThreads), 0, stream, at);
    hipLaunchKernelGGL((dot_attention_sum_pieces_kernel<V, 2>), pgrid, dim3(kThreads), 0, stream,
                       at);
  }
  DGLHIP_CHECK(hipGetLastError() == hipSuccess, "dot attention dk / dv launch failed");
}

}  // namespace

}  // namespace dglhip

using namespace dglhip;

extern "C" {

int64_t dglhip_dot_attention_workspace_bytes(int64_t num_rows, int64_t nnz, int64_t num_heads,
                                             int64_t head_dim, int64_t max_row_len) {
  if (num_rows <= 0 || num_heads <= 0 || head_dim <= 0 || !has_pieces(nnz, max_row_len, kChunk))
    return 0;
  return 2 * num_blocks(nnz, kChunk) * (2 * num_heads * head_dim + 2 * num_heads) * 4;
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
  with_vec(V, [&](auto v) { forward_v<decltype(v)::value>(a, st); });
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
  with_vec(V, [&](auto v) { backward_v<decltype(v)::value>(aq, at, st); });
  API_END();
}

}  // extern "C"
