// GATv2 attention over the in-edges of a graph (Brody et al., "How Attentive
// are Graph Attention Networks?"), fused: for every destination r (a row of
// the CSR), head h and in-edge slot j with source u_j,
//
//   z_j[d] = fs[u_j,h,d] + fd[r,h,d]
//   s_j    = sum_d attn[h,d] * lrelu(z_j[d]),   lrelu(z) = z > 0 ? z : slope * z
//   a_j    = expf(s_j - max_j s_j) / sum_j expf(s_j - max_j s_j)
//   out[r,h,:] = sum_j a_j fs[u_j,h,:],   lse[r,h] = max_j s_j + logf(sum_j ...)
//
// in one pass over the CSR. The score and the value read the same gathered
// source row: one gather per edge, where dot_attention.hip needs two (k and
// v). The backward takes two walks, both recomputing z_j, s_j and a_j =
// expf(s_j - lse); with dp_j = <dout[r], fs_j>, ds_j = a_j (dp_j - delta[r]),
// delta = <dout, out> and g'(z) = z > 0 ? 1 : slope,
//
//   dfd[r,h,d]  = attn[d] * sum_j ds_j g'(z_j[d])               over the CSR,
//   dattn[h,d]  = sum over all edges of ds_j lrelu(z_j[d])      in the same walk,
//   dfs[u,h,d]  = sum over u's out-edges of (a_j dout[r,d] + ds_j attn[d] g'(z_j[d]))
//                                                    over the transposed CSR.
//
// Nothing of the size of the edge set is stored.
//
// Why no MFMA. Per edge the work is elementwise on one gathered row of fs
// and one row of fd, then a weighted sum: no product of two matrices at all,
// and, as in dot_attention.hip, two destinations share no source rows that a
// tile could hold. The kernels are bound by the gathers and stay on the
// vector unit.
//
// Lane map: attention_walk.h's, as dot_attention.hip. fd[r] and attn[h] (in the
// transposed walk fs[u] and attn[h]) are loaded once per wave and stay in
// registers; lanes past D hold zeros, of attn too. A score is summed per lane
// over its VEC features (lane_score: one product, then fmas, in feature order)
// and across the head's lanes by head_sum's butterfly (attention_lanes.h); the
// three walks use the same chain, so they get the same bits for s_j.
//
// The walk: attention_walk.h's; the slots run in batches whose single gather
// per slot (three in the transposed walk: fd, dout, and lse with delta) is
// issued before first use. Forward, per batch: the elementwise scores, one
// butterfly, then the online softmax's step with fs_j as the value row. The
// batch sizes (DGLHIP_GATV2_BATCH*) are the largest of 8, 16, 32 (the sizes
// that divide a trip's 64 ids) whose resource report shows no scratch in any
// instantiation and, at VEC 4, the 4 waves per SIMD of dot_attention.hip's
// forward: 16 slots forward (one gathered row a slot, where that kernel's 8
// hold two), 8 in the dfd walk (it also keeps dout and two accumulators; 16
// halve its waves, the same rows in flight) and 8 in the dfs walk (two rows
// a slot).
//
// Long rows: attention_walk.h's pieces, cut at the multiples of
// DGLHIP_GATV2_CHUNK.
//
// dattn is the one output that sums across rows. Every wave of the dfd walk
// leaves its partial (of its schedule item, or of its piece; zeros where it
// walks nothing) in the workspace: R + 2 G slots of H D floats, all written
// on every call. Two kernels add them in slot order: kParts consecutive
// ranges of slots, a thread per element, then the ranges' sums in order.
//
// No atomics; every output element has one writer: the same bits on every call.
#include "../../include/dgl_hip.h"
#include "attention_walk.h"

#include <hip/hip_runtime.h>

#include <cmath>

namespace dglhip {

namespace {

constexpr int64_t kChunk = DGLHIP_GATV2_CHUNK;
constexpr int kBatchFwd = DGLHIP_GATV2_BATCH;
constexpr int kBatchDfd = DGLHIP_GATV2_BATCH_DFD;
constexpr int kBatchDfs = DGLHIP_GATV2_BATCH_DFS;
constexpr int64_t kParts = 1024;  // ranges of dattn partials summed side by side

struct Args : Walk {
  float slope;
  const float *fs, *fd, *attn;  // fs by source, fd by destination, attn (H, D)
  const float *dout, *out;      // by destination (backward)
  const float *lse, *delta;     // (destinations, H), read (backward)
  float* o0;                    // out | dfd | dfs
  float* stat;                  // lse (forward) or delta (the dfd walk), written
  float *ws0, *wsml;            // the pieces: 2 G rows of H D floats, 2 G H (m, l) pairs
  float *part, *part2;          // dattn: a partial per slot, a sum per range of slots
  float* dattn;
  int64_t slots, per, nparts;   // dattn partials, slots a range, ranges
};

__device__ __forceinline__ float lrelu(float z, float slope) { return z > 0.0f ? z : slope * z; }

// torch's leaky_relu backward: the slope at z <= 0, z == 0 included
__device__ __forceinline__ float lrelu_grad(float z, float slope) {
  return z > 0.0f ? 1.0f : slope;
}

// a lane's share of a score, the one chain of all three walks: z = fs + fd,
// attn[0] lrelu(z[0]), then fmas in feature order
template <int VEC>
__device__ __forceinline__ float lane_score(const float (&fs)[VEC], const float (&fd)[VEC],
                                            const float (&at)[VEC], float slope) {
  float t = at[0] * lrelu(fs[0] + fd[0], slope);
#pragma unroll
  for (int c = 1; c < VEC; ++c) t = __builtin_fmaf(at[c], lrelu(fs[c] + fd[c], slope), t);
  return t;
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <int VEC>
__device__ __forceinline__ void fwd_range(const Args& a, const Place& p, int lane,
                                          const float (&fdv)[VEC], const float (&atv)[VEC],
                                          int64_t k0, int64_t k1, float& m, float& l,
                                          float (&acc)[VEC]) {
  const int64_t F = a.H * a.D;
  batch_ids<kBatchFwd>(a.indices, a.C, k0, k1, lane, [&](const int (&u)[kBatchFwd], int n) {
    float ff[kBatchFwd][VEC], s[kBatchFwd];
#pragma unroll
    for (int i = 0; i < kBatchFwd; ++i) row_load<VEC>(a.fs, u[i], F, p, ff[i]);
#pragma unroll
    for (int i = 0; i < kBatchFwd; ++i) s[i] = lane_score<VEC>(ff[i], fdv, atv, a.slope);
    head_sum<kBatchFwd>(s, a.lph_shift);
    softmax_step<kBatchFwd, VEC>(s, n, ff, m, l, acc);
  });
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void gatv2_fwd_rows_kernel(Args a) {
  const int lane = threadIdx.x & 63;
  int64_t it, row, tile, beg, end;
  if (wave_row<kChunk>(a, it, row, tile, beg, end) != kWalk) return;  // the whole wave
  const Place p = place_of<VEC>(a, tile, lane);
  float fdv[VEC], atv[VEC], acc[VEC];
  row_load<VEC>(a.fd, row, a.H * a.D, p, fdv);
  row_load<VEC>(a.attn, 0, 0, p, atv);
  float m = -INFINITY, l = 0.0f;
  zero<VEC>(acc);
  fwd_range<VEC>(a, p, lane, fdv, atv, beg, end, m, l, acc);
  fwd_store<VEC>(a, p, row, beg == end, m, l, acc);
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void gatv2_fwd_piece_kernel(Args a) {
  const int lane = threadIdx.x & 63;
  Piece pc;
  int64_t tile;
  if (wave_piece<kChunk>(a, lane, pc, tile) != kWalk) return;  // the whole wave
  const Place p = place_of<VEC>(a, tile, lane);
  float fdv[VEC], atv[VEC], acc[VEC];
  row_load<VEC>(a.fd, pc.row, a.H * a.D, p, fdv);
  row_load<VEC>(a.attn, 0, 0, p, atv);
  float m = -INFINITY, l = 0.0f;
  zero<VEC>(acc);
  fwd_range<VEC>(a, p, lane, fdv, atv, pc.k0, pc.k1, m, l, acc);
  if (p.live) store_vec<VEC>(a.ws0 + pc.item * a.H * a.D + p.foff, acc);
  if (p.first) {
    a.wsml[(pc.item * a.H + p.head) * 2] = m;
    a.wsml[(pc.item * a.H + p.head) * 2 + 1] = l;
  }
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void gatv2_fwd_combine_kernel(Args a) {
  fwd_combine<VEC, kChunk>(a);
}

// ---------------------------------------------------------------------------
// backward over the forward CSR: delta, dfd and the dattn partials
// ---------------------------------------------------------------------------
// what a destination's wave holds: fd, and dout, lse and delta of its head
template <int VEC>
struct DstRow : DstGrad<VEC> {
  float fd[VEC];
};

template <int VEC>
__device__ __forceinline__ DstRow<VEC> dst_row(const Args& a, const Place& p, int64_t row) {
  DstRow<VEC> d;
  row_load<VEC>(a.fd, row, a.H * a.D, p, d.fd);
  dst_grad<VEC>(a, p, row, d);
  return d;
}

// gs[d] += ds_j g'(z_j[d]) and da[d] += ds_j lrelu(z_j[d]) over the slots
template <int VEC>
__device__ __forceinline__ void dfd_range(const Args& a, const Place& p, int lane,
                                          const DstRow<VEC>& d, const float (&atv)[VEC],
                                          int64_t k0, int64_t k1, float (&gs)[VEC],
                                          float (&da)[VEC]) {
  const int64_t F = a.H * a.D;
  batch_ids<kBatchDfd>(a.indices, a.C, k0, k1, lane, [&](const int (&u)[kBatchDfd], int n) {
    float ff[kBatchDfd][VEC], s[kBatchDfd], dp[kBatchDfd];
#pragma unroll
    for (int i = 0; i < kBatchDfd; ++i) row_load<VEC>(a.fs, u[i], F, p, ff[i]);
#pragma unroll
    for (int i = 0; i < kBatchDfd; ++i) {
      s[i] = lane_score<VEC>(ff[i], d.fd, atv, a.slope);
      dp[i] = lane_dot<VEC>(d.dout, ff[i]);
    }
    head_sum<kBatchDfd>(s, a.lph_shift);
    head_sum<kBatchDfd>(dp, a.lph_shift);
#pragma unroll
    for (int i = 0; i < kBatchDfd; ++i) {
      if (i < n) {
        const float ds = expf(s[i] - d.lse) * (dp[i] - d.delta);
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
          const float z = ff[i][c] + d.fd[c];
          gs[c] = __builtin_fmaf(ds, lrelu_grad(z, a.slope), gs[c]);
          da[c] = __builtin_fmaf(ds, lrelu(z, a.slope), da[c]);
        }
      }
    }
  });
}

// dfd (or a piece's share of it) = attn * gs
template <int VEC>
__device__ __forceinline__ void dfd_store(float* at, const Place& p, const float (&atv)[VEC],
                                          const float (&gs)[VEC]) {
  float o[VEC];
#pragma unroll
  for (int c = 0; c < VEC; ++c) o[c] = atv[c] * gs[c];
  if (p.live) store_vec<VEC>(at + p.foff, o);
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void gatv2_dfd_rows_kernel(Args a) {
  const int lane = threadIdx.x & 63;
  int64_t it, row, tile, beg, end;
  const Found found = wave_row<kChunk>(a, it, row, tile, beg, end);
  if (found == kPast) return;  // the whole wave
  const Place p = place_of<VEC>(a, tile, lane);
  const int64_t F = a.H * a.D;
  float gs[VEC], da[VEC];
  zero<VEC>(gs);
  zero<VEC>(da);
  if (found == kWalk) {
    float atv[VEC];
    row_load<VEC>(a.attn, 0, 0, p, atv);
    const DstRow<VEC> d = dst_row<VEC>(a, p, row);
    if (p.first) a.stat[row * a.H + p.head] = d.delta;
    dfd_range<VEC>(a, p, lane, d, atv, beg, end, gs, da);
    dfd_store<VEC>(a.o0 + row * F, p, atv, gs);
  }
  // (the slot of every item is written: zeros where the pieces hold the row)
  if (p.live) store_vec<VEC>(a.part + it * F + p.foff, da);
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void gatv2_dfd_piece_kernel(Args a) {
  const int lane = threadIdx.x & 63;
  Piece pc;
  int64_t tile;
  const Found found = wave_piece<kChunk>(a, lane, pc, tile);
  if (found == kPast) return;  // the whole wave
  const Place p = place_of<VEC>(a, tile, lane);
  const int64_t F = a.H * a.D;
  float gs[VEC], da[VEC];
  zero<VEC>(gs);
  zero<VEC>(da);
  if (found == kWalk) {
    float atv[VEC];
    row_load<VEC>(a.attn, 0, 0, p, atv);
    const DstRow<VEC> d = dst_row<VEC>(a, p, pc.row);
    if (p.first && pc.item == pc.first) a.stat[pc.row * a.H + p.head] = d.delta;
    dfd_range<VEC>(a, p, lane, d, atv, pc.k0, pc.k1, gs, da);
    dfd_store<VEC>(a.ws0 + pc.item * F, p, atv, gs);
  }
  if (p.live) store_vec<VEC>(a.part + (a.R + pc.item) * F + p.foff, da);
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void gatv2_sum_pieces_kernel(Args a) {
  sum_pieces<VEC, 1, kChunk>(a);
}

// dattn, first level: a thread per element (h, d) adds the partials of range
// blockIdx.y of the slots, in slot order
__global__ __launch_bounds__(kThreads) void gatv2_dattn_ranges_kernel(Args a) {
  const int64_t F = a.H * a.D;
  const int64_t f = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  const int64_t range = blockIdx.y;
  if (f >= F || range >= a.nparts) return;
  const int64_t s0 = range * a.per;
  const int64_t s1 = s0 + a.per < a.slots ? s0 + a.per : a.slots;
  float t = 0.0f;
  for (int64_t s = s0; s < s1; ++s) t = t + a.part[s * F + f];
  a.part2[range * F + f] = t;
}

// second level: the ranges' sums in order
__global__ __launch_bounds__(kThreads) void gatv2_dattn_sum_kernel(Args a) {
  const int64_t F = a.H * a.D;
  const int64_t f = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (f >= F) return;
  float t = 0.0f;
  for (int64_t r = 0; r < a.nparts; ++r) t = t + a.part2[r * F + f];
  a.dattn[f] = t;
}

// ---------------------------------------------------------------------------
// backward over the transposed CSR: dfs, a wave per (source, head tile)
// ---------------------------------------------------------------------------
// val[d] += a_j dout[r,d] (the value path) and sc[d] += ds_j g'(z_j[d]) (the
// score path) over the out-edges; the ids handed out are destinations
template <int VEC>
__device__ __forceinline__ void dfs_range(const Args& a, const Place& p, int lane,
                                          const float (&fsv)[VEC], const float (&atv)[VEC],
                                          int64_t k0, int64_t k1, float (&val)[VEC],
                                          float (&sc)[VEC]) {
  const int64_t F = a.H * a.D;
  batch_ids<kBatchDfs>(a.indices, a.C, k0, k1, lane, [&](const int (&r)[kBatchDfs], int n) {
    float dd[kBatchDfs][VEC], go[kBatchDfs][VEC];
    float ls[kBatchDfs], de[kBatchDfs], s[kBatchDfs], dp[kBatchDfs];
#pragma unroll
    for (int i = 0; i < kBatchDfs; ++i) row_load<VEC>(a.fd, r[i], F, p, dd[i]);
#pragma unroll
    for (int i = 0; i < kBatchDfs; ++i) row_load<VEC>(a.dout, r[i], F, p, go[i]);
#pragma unroll
    for (int i = 0; i < kBatchDfs; ++i) {
      // (one 4-byte load for the lanes of a head)
      ls[i] = a.lse[r[i] * a.H + p.hsafe];
      de[i] = a.delta[r[i] * a.H + p.hsafe];
    }
#pragma unroll
    for (int i = 0; i < kBatchDfs; ++i) {
      s[i] = lane_score<VEC>(fsv, dd[i], atv, a.slope);
      dp[i] = lane_dot<VEC>(go[i], fsv);
    }
    head_sum<kBatchDfs>(s, a.lph_shift);
    head_sum<kBatchDfs>(dp, a.lph_shift);
#pragma unroll
    for (int i = 0; i < kBatchDfs; ++i) {
      if (i < n) {
        const float e = expf(s[i] - ls[i]);
        const float ds = e * (dp[i] - de[i]);
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
          val[c] = __builtin_fmaf(e, go[i][c], val[c]);
          sc[c] = __builtin_fmaf(ds, lrelu_grad(fsv[c] + dd[i][c], a.slope), sc[c]);
        }
      }
    }
  });
}

template <int VEC, bool PIECE>
__global__ __launch_bounds__(kThreads) void gatv2_dfs_kernel(Args a) {
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
  float fsv[VEC], atv[VEC], val[VEC], sc[VEC], o[VEC];
  row_load<VEC>(a.fs, row, F, p, fsv);
  row_load<VEC>(a.attn, 0, 0, p, atv);
  zero<VEC>(val);
  zero<VEC>(sc);
  dfs_range<VEC>(a, p, lane, fsv, atv, beg, end, val, sc);
#pragma unroll
  for (int c = 0; c < VEC; ++c) o[c] = __builtin_fmaf(atv[c], sc[c], val[c]);
  if (p.live) store_vec<VEC>((PIECE ? a.ws0 : a.o0) + at * F + p.foff, o);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// The workspace, in floats: the pieces' rows [0, ml), their (m, l) pairs
// [ml, part), and for the backward the dattn partials [part, part2) and the
// ranges' sums [part2, total). One set of pieces serves both walks of the
// backward (they follow each other on the stream).
struct Layout {
  int64_t G, Gq;  // blocks when either CSR has pieces, when the forward one has
  int64_t ml, part, part2, total, slots;
};

Layout layout_of(int64_t R, int64_t nnz, int64_t H, int64_t D, int64_t max_row_len,
                 int64_t max_col_len, bool backward) {
  Layout w = {};
  const int64_t F = H * D;
  w.Gq = has_pieces(nnz, max_row_len, kChunk) ? num_blocks(nnz, kChunk) : 0;
  w.G = (w.Gq || (backward && has_pieces(nnz, max_col_len, kChunk))) ? num_blocks(nnz, kChunk) : 0;
  w.ml = 2 * w.G * F;
  w.part = w.ml + 4 * w.G * H;
  w.slots = backward ? R + 2 * w.Gq : 0;
  w.part2 = w.part + w.slots * F;
  w.total = w.part2 + (backward ? kParts * F : 0);
  return w;
}

template <int V>
void forward_v(const Args& a, hipStream_t stream) {
  hipLaunchKernelGGL((gatv2_fwd_rows_kernel<V>), waves_grid(a.R * a.tiles), dim3(kThreads), 0,
                     stream, a);
  if (a.G > 0) {
    const dim3 pgrid = waves_grid(2 * a.G * a.tiles);
    hipLaunchKernelGGL((gatv2_fwd_piece_kernel<V>), pgrid, dim3(kThreads), 0, stream, a);
    hipLaunchKernelGGL((gatv2_fwd_combine_kernel<V>), pgrid, dim3(kThreads), 0, stream, a);
  }
  DGLHIP_CHECK(hipGetLastError() == hipSuccess, "gatv2 attention launch failed");
}

template <int V>
void backward_v(const Args& aq, const Args& at, hipStream_t stream) {
  const int64_t F = aq.H * aq.D;
  if (aq.R > 0)
    hipLaunchKernelGGL((gatv2_dfd_rows_kernel<V>), waves_grid(aq.R * aq.tiles), dim3(kThreads), 0,
                       stream, aq);
  if (aq.G > 0) {
    const dim3 pgrid = waves_grid(2 * aq.G * aq.tiles);
    hipLaunchKernelGGL((gatv2_dfd_piece_kernel<V>), pgrid, dim3(kThreads), 0, stream, aq);
    hipLaunchKernelGGL((gatv2_sum_pieces_kernel<V>), pgrid, dim3(kThreads), 0, stream, aq);
  }
  const unsigned fblocks = static_cast<unsigned>((F + kThreads - 1) / kThreads);
  if (aq.nparts > 0)
    hipLaunchKernelGGL(gatv2_dattn_ranges_kernel, dim3(fblocks, static_cast<unsigned>(aq.nparts)),
                       dim3(kThreads), 0, stream, aq);
  hipLaunchKernelGGL(gatv2_dattn_sum_kernel, dim3(fblocks), dim3(kThreads), 0, stream, aq);
  DGLHIP_CHECK(hipGetLastError() == hipSuccess, "gatv2 attention dfd launch failed");
  if (at.R == 0) return;
  // (after dfd on the stream: both walks' pieces go through one workspace)
  hipLaunchKernelGGL((gatv2_dfs_kernel<V, false>), waves_grid(at.R * at.tiles), dim3(kThreads), 0,
                     stream, at);
  if (at.G > 0) {
    const dim3 pgrid = waves_grid(2 * at.G * at.tiles);
    hipLaunchKernelGGL((gatv2_dfs_kernel<V, true>), pgrid, dim3(kThreads), 0, stream, at);
    hipLaunchKernelGGL((gatv2_sum_pieces_kernel<V>), pgrid, dim3(kThreads), 0, stream, at);
  }
  DGLHIP_CHECK(hipGetLastError() == hipSuccess, "gatv2 attention dfs launch failed");
}

}  // namespace

}  // namespace dglhip

using namespace dglhip;

extern "C" {

int64_t dglhip_gatv2_attention_workspace_bytes(int64_t num_rows, int64_t nnz, int64_t num_heads,
                                               int64_t head_dim, int64_t max_row_len,
                                               int64_t max_col_len, int backward) {
  if (num_rows < 0 || nnz < 0 || num_heads <= 0 || head_dim <= 0) return 0;
  return layout_of(num_rows, nnz, num_heads, head_dim, max_row_len, max_col_len, backward != 0)
             .total * 4;
}

int dglhip_gatv2_attention_device(int64_t num_rows, int64_t num_cols, int64_t nnz,
                                  int64_t num_heads, int64_t head_dim, const int64_t* indptr,
                                  const int32_t* indices, const int32_t* row_order,
                                  const float* fs, const float* fd, const float* attn,
                                  float negative_slope, float* out, float* lse,
                                  int64_t max_row_len, void* workspace, void* stream) {
  API_BEGIN();
  check_sizes(num_rows, num_cols, nnz, num_heads, head_dim);
  if (num_rows == 0 || num_heads == 0 || head_dim == 0) return 0;
  DGLHIP_CHECK(indptr && fd && attn && out && lse && (nnz == 0 || (indices && fs)),
               "null pointer argument");
  const Layout w = layout_of(num_rows, nnz, num_heads, head_dim, max_row_len, 0, false);
  DGLHIP_CHECK(w.total == 0 || workspace, "rows longer than a chunk need the workspace");
  Args a = {};
  a.R = num_rows; a.C = num_cols; a.nnz = nnz; a.H = num_heads; a.D = head_dim;
  a.slope = negative_slope;
  a.indptr = indptr; a.indices = indices; a.row_order = row_order;
  a.fs = fs; a.fd = fd; a.attn = attn;
  a.o0 = out; a.stat = lse;
  a.G = w.G;
  a.ws0 = static_cast<float*>(workspace);
  a.wsml = a.ws0 + w.ml;
  const int V = vec_of(head_dim, {fs, fd, attn, out, a.G ? workspace : nullptr});
  lane_map(a, V);
  hipStream_t st = static_cast<hipStream_t>(stream);
  with_vec(V, [&](auto v) { forward_v<decltype(v)::value>(a, st); });
  API_END();
}

int dglhip_gatv2_attention_bwd_device(int64_t num_rows, int64_t num_cols, int64_t nnz,
                                      int64_t num_heads, int64_t head_dim, const int64_t* indptr,
                                      const int32_t* indices, const int32_t* row_order,
                                      const int64_t* t_indptr, const int32_t* t_indices,
                                      const int32_t* t_row_order, const float* fs,
                                      const float* fd, const float* attn, const float* out,
                                      const float* lse, const float* dout, float negative_slope,
                                      float* delta, float* dfs, float* dfd, float* dattn,
                                      int64_t max_row_len, int64_t max_col_len, void* workspace,
                                      void* stream) {
  API_BEGIN();
  check_sizes(num_rows, num_cols, nnz, num_heads, head_dim);
  if (num_heads == 0 || head_dim == 0) return 0;
  DGLHIP_CHECK(indptr && t_indptr && attn && dattn && workspace &&
                   (num_rows == 0 || (fd && out && lse && dout && delta && dfd)) &&
                   (num_cols == 0 || (fs && dfs)) && (nnz == 0 || (indices && t_indices)),
               "null pointer argument");
  const Layout w = layout_of(num_rows, nnz, num_heads, head_dim, max_row_len, max_col_len, true);
  float* ws = static_cast<float*>(workspace);
  Args aq = {};
  aq.R = num_rows; aq.C = num_cols; aq.nnz = nnz; aq.H = num_heads; aq.D = head_dim;
  aq.slope = negative_slope;
  aq.indptr = indptr; aq.indices = indices; aq.row_order = row_order;
  aq.fs = fs; aq.fd = fd; aq.attn = attn; aq.dout = dout; aq.out = out; aq.lse = lse;
  aq.o0 = dfd; aq.stat = delta; aq.dattn = dattn;
  aq.G = w.Gq;
  aq.ws0 = ws; aq.wsml = ws + w.ml; aq.part = ws + w.part; aq.part2 = ws + w.part2;
  aq.slots = w.slots;
  aq.per = (w.slots + kParts - 1) / kParts;
  aq.nparts = aq.per ? (w.slots + aq.per - 1) / aq.per : 0;
  Args at = aq;
  at.R = num_cols; at.C = num_rows;
  at.indptr = t_indptr; at.indices = t_indices; at.row_order = t_row_order;
  at.delta = delta; at.o0 = dfs; at.stat = nullptr;
  at.G = has_pieces(nnz, max_col_len, kChunk) ? w.G : 0;
  const int V = vec_of(head_dim, {fs, fd, attn, out, dout, dfs, dfd, workspace});
  lane_map(aq, V);
  lane_map(at, V);
  hipStream_t st = static_cast<hipStream_t>(stream);
  with_vec(V, [&](auto v) { backward_v<decltype(v)::value>(aq, at, st); });
  API_END();
}

}  // extern "C"
