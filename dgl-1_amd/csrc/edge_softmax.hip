// Edge softmax: the softmax of per-edge scores over the slots of each CSR row
// (the in-edges of a node, the out-edges over the transpose, the nodes or
// edges of each graph of a batch) and its backward.
//
//   forward   m = max_k x[k, h], e_k = expf(x[k, h] - m), s = sum_k e_k,
//             y[k, h] = e_k / s
//   backward  t = sum_k y[k, h] dy[k, h], dx[k, h] = y[k, h] (dy[k, h] - t)
//
// over the slots k of a row, per column h; slot k is row eid[k] of x (row k
// when eid is NULL), and y / dx are stored where x was read from.
//
// Lane map. A slot is taken by LPS lanes, each V columns of it (V = 4 with
// 16-byte accesses when H % 4 == 0 and the tensors are 16-byte aligned, else
// 1; LPS = min(64, pow2 >= H / V); H > 64 V columns are tiled over waves), so
// a wave has S = 64 / LPS slot lanes and, without eid, its lanes read
// consecutive (slot, column) pairs of a row. The max and the sums run first
// down a lane's own slots, then across the slot lanes that hold the same
// columns, as a butterfly of shuffles at strides LPS, 2 LPS, ...: both
// partners of a stage add the same two numbers, so every lane of a row ends
// with the same bits, whatever the launch.
//
// Tiers, from the sizes alone (no host sync, no data-dependent geometry):
//  - Rows of at most DGLHIP_EDGE_SOFTMAX_CHUNK slots. A wave takes W rows of
//    the schedule (W a power of two from the mean row length: 64 rows of
//    Cora's four edges, one row of Reddit's 490), reads their lengths, and
//    gives each row a team of T slot lanes, T the power of two that covers
//    the longest of them (at most S): S / T rows run side by side. A row of
//    at most T K slots (K = 16 steps, 8 in the backward, which holds y and
//    dy) stays in registers and is read from memory once; a longer one takes
//    three passes (max, sum, store; two in the backward), the re-reads from L2.
//  - Longer rows are cut where they cross the multiples of the chunk: block g
//    is slots [g C, (g + 1) C), and it meets at most two long rows, the one
//    that holds its first slot and one that starts inside it. Each such piece
//    is one workgroup's, a quarter of the block per wave (read once, into
//    registers, up to H = 16 at V = 4), the waves' maxima and sums combined
//    through LDS in wave order; the piece's (max, sum) goes to slot 2 g or
//    2 g + 1 of the workspace, one thread per (row, column) combines a row's
//    pieces in block order, m = max m_g, s = sum s_g expf(m_g - m), and leaves
//    the result in the row's first slot, and a third launch stores the pieces'
//    values.
//
// No atomics; every output element is written exactly once.
#include "../../include/dgl_hip.h"
#include "common.h"
#include "launch.h"

#include <hip/hip_runtime.h>

#include <cmath>

namespace dglhip {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int64_t kChunk = DGLHIP_EDGE_SOFTMAX_CHUNK;

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int V>
__device__ __forceinline__ void load_cols(const float* p, float (&v)[V]) {
  if constexpr (V == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  } else {
    v[0] = *p;
  }
}

template <int V>
__device__ __forceinline__ void store_cols(float* p, const float (&v)[V]) {
  if constexpr (V == 4) {
    f32x4 t;
    t[0] = v[0]; t[1] = v[1]; t[2] = v[2]; t[3] = v[3];
    *reinterpret_cast<f32x4*>(p) = t;
  } else {
    *p = v[0];
  }
}

__device__ __forceinline__ int64_t clampi(int64_t v, int64_t lo, int64_t hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

// torch's max: a NaN on either side wins (fmaxf would drop it)
__device__ __forceinline__ float nanmax(float a, float b) { return (a > b || a != a) ? a : b; }

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

struct Args {
  int64_t R, nnz, H;
  int64_t G;      // blocks of kChunk slots (0: no row is longer than a chunk)
  int64_t W;      // rows of the schedule per wave
  int64_t tiles;  // column tiles per item
  int lps_shift;  // log2 of the lanes per slot
  const int64_t* indptr;
  const int64_t* eid;
  const int32_t* row_order;
  const float* x;   // the scores; in the backward the forward's y
  const float* dy;  // backward only
  float* out;
  float* partial;  // 2 G slots of 2 H floats: (m, s) per column, (t, -) in the backward
};

// steps of a row a lane keeps in registers
template <bool BWD>
constexpr int kRegSteps = BWD ? 8 : 16;

// what a lane knows of its place: V columns from col0 of the slots q, q + T, ...
struct Place {
  int lps, T, q, l;
  int64_t col0;
  bool colok;
};

template <int V>
__device__ __forceinline__ void team_max(float (&m)[V], const Place& p) {
  for (int o = p.lps; o < p.lps * p.T; o <<= 1) {
#pragma unroll
    for (int c = 0; c < V; ++c) m[c] = nanmax(m[c], __shfl_xor(m[c], o));
  }
}

template <int V>
__device__ __forceinline__ void team_sum(float (&s)[V], const Place& p) {
  for (int o = p.lps; o < p.lps * p.T; o <<= 1) {
#pragma unroll
    for (int c = 0; c < V; ++c) s[c] = s[c] + __shfl_xor(s[c], o);
  }
}

// A piece is a workgroup's: its kWaves waves take a quarter each, and their
// maxima (sums) meet here, through LDS, in wave order: the same bits in
// every lane. Every thread of the workgroup must call it.
template <int V, bool MAX>
__device__ __forceinline__ void waves_combine(float (&v)[V], const Place& p, float* sm) {
  const int wave = threadIdx.x >> 6;
  if (p.q == 0) {
#pragma unroll
    for (int c = 0; c < V; ++c) sm[(wave * 64 + p.l) * V + c] = v[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < V; ++c) {
    float r = sm[p.l * V + c];
    for (int w = 1; w < kWaves; ++w) {
      const float t = sm[(w * 64 + p.l) * V + c];
      r = MAX ? nanmax(r, t) : r + t;
    }
    v[c] = r;
  }
  __syncthreads();  // sm is written again
}

__device__ __forceinline__ int64_t slot_offset(const Args& a, int64_t k) {
  return (a.eid ? a.eid[k] : k) * a.H;
}

// The team's row (or piece of one): slots [beg, beg + len), nsteps = the
// steps of the longest row of the wave (the same in every lane, so every lane
// reaches the shuffles). pslot: the piece's workspace slot (its max and sum
// are stored and nothing else), or NULL (the row is finished here).
template <int V, bool BWD, bool WG>
__device__ __forceinline__ void team_range(const Args& a, const Place& p, int64_t beg,
                                           int64_t len, int64_t nsteps, float* pslot,
                                           float* sm) {
  constexpr int K = kRegSteps<BWD>;
  const float ninf = -INFINITY;
  float m[V], s[V];
#pragma unroll
  for (int c = 0; c < V; ++c) {
    m[c] = ninf;
    s[c] = 0.0f;
  }
  const float* xp = a.x + p.col0;
  float* op = a.out + p.col0;
  if (nsteps <= K) {
    // the row in registers: one read
    float v[K][V];
    float g[BWD ? K : 1][V];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      if (j < nsteps) {
        const int64_t k = p.q + int64_t(j) * p.T;
        if (p.colok && k < len) {
          const int64_t off = slot_offset(a, beg + k);
          load_cols<V>(xp + off, v[j]);
          if constexpr (BWD) load_cols<V>(a.dy + p.col0 + off, g[j]);
        } else {
#pragma unroll
          for (int c = 0; c < V; ++c) {
            v[j][c] = BWD ? 0.0f : ninf;
            if constexpr (BWD) g[j][c] = 0.0f;
          }
        }
      }
    }
    if constexpr (!BWD) {
#pragma unroll
      for (int j = 0; j < K; ++j) {
        if (j < nsteps) {
#pragma unroll
          for (int c = 0; c < V; ++c) m[c] = nanmax(m[c], v[j][c]);
        }
      }
      team_max<V>(m, p);
      if constexpr (WG) waves_combine<V, true>(m, p, sm);
#pragma unroll
      for (int j = 0; j < K; ++j) {
        if (j < nsteps) {
          const bool live = p.colok && p.q + int64_t(j) * p.T < len;
#pragma unroll
          for (int c = 0; c < V; ++c) {
            v[j][c] = expf(v[j][c] - m[c]);
            s[c] = s[c] + (live ? v[j][c] : 0.0f);
          }
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < K; ++j) {
        if (j < nsteps) {
#pragma unroll
          for (int c = 0; c < V; ++c) s[c] = s[c] + v[j][c] * g[j][c];
        }
      }
    }
    team_sum<V>(s, p);
    if constexpr (WG) waves_combine<V, false>(s, p, sm);
    if (!pslot) {
#pragma unroll
      for (int j = 0; j < K; ++j) {
        if (j < nsteps) {
          const int64_t k = p.q + int64_t(j) * p.T;
          if (p.colok && k < len) {
            float o[V];
#pragma unroll
            for (int c = 0; c < V; ++c)
              o[c] = BWD ? v[j][c] * (g[j][c] - s[c]) : v[j][c] / s[c];
            store_cols<V>(op + slot_offset(a, beg + k), o);
          }
        }
      }
    }
  } else {
    // passes over the row, the re-reads from L2
    if constexpr (!BWD) {
      if (p.colok) {
#pragma unroll 4
        for (int64_t k = p.q; k < len; k += p.T) {
          float v[V];
          load_cols<V>(xp + slot_offset(a, beg + k), v);
#pragma unroll
          for (int c = 0; c < V; ++c) m[c] = nanmax(m[c], v[c]);
        }
      }
      team_max<V>(m, p);
      if constexpr (WG) waves_combine<V, true>(m, p, sm);
    }
    if (p.colok) {
#pragma unroll 4
      for (int64_t k = p.q; k < len; k += p.T) {
        const int64_t off = slot_offset(a, beg + k);
        float v[V];
        load_cols<V>(xp + off, v);
        if constexpr (BWD) {
          float g[V];
          load_cols<V>(a.dy + p.col0 + off, g);
#pragma unroll
          for (int c = 0; c < V; ++c) s[c] = s[c] + v[c] * g[c];
        } else {
#pragma unroll
          for (int c = 0; c < V; ++c) s[c] = s[c] + expf(v[c] - m[c]);
        }
      }
    }
    team_sum<V>(s, p);
    if constexpr (WG) waves_combine<V, false>(s, p, sm);
    if (!pslot && p.colok) {
#pragma unroll 4
      for (int64_t k = p.q; k < len; k += p.T) {
        const int64_t off = slot_offset(a, beg + k);
        float v[V], o[V];
        load_cols<V>(xp + off, v);
        if constexpr (BWD) {
          float g[V];
          load_cols<V>(a.dy + p.col0 + off, g);
#pragma unroll
          for (int c = 0; c < V; ++c) o[c] = v[c] * (g[c] - s[c]);
        } else {
#pragma unroll
          for (int c = 0; c < V; ++c) o[c] = expf(v[c] - m[c]) / s[c];
        }
        store_cols<V>(op + off, o);
      }
    }
  }
  if (pslot && p.colok && p.q == 0 && (!WG || threadIdx.x < 64)) {
#pragma unroll
    for (int c = 0; c < V; ++c) {
      pslot[(p.col0 + c) * 2] = BWD ? s[c] : m[c];
      pslot[(p.col0 + c) * 2 + 1] = BWD ? 0.0f : s[c];
    }
  }
}


template <int V>
__device__ __forceinline__ Place place_of(const Args& a, int64_t tile, int lane) {
  Place p;
  p.lps = 1 << a.lps_shift;
  p.T = 64 >> a.lps_shift;
  p.q = lane >> a.lps_shift;
  p.l = lane & (p.lps - 1);
  p.col0 = (tile * p.lps + p.l) * V;
  p.colok = p.col0 < a.H;
  return p;
}

// Rows of at most a chunk of slots: W rows of the schedule per wave, the waves
// of a workgroup each on their own (no barrier).
template <int V, bool BWD>
__global__ __launch_bounds__(kThreads) void edge_softmax_rows_kernel(Args a) {
  const int64_t id = block_linear() * kWaves + (threadIdx.x >> 6);
  const int64_t wave = id / a.tiles, tile = id - wave * a.tiles;
  const int lane = threadIdx.x & 63;
  const int64_t i0 = wave * a.W;
  if (i0 >= a.R) return;  // the whole wave
  Place p = place_of<V>(a, tile, lane);
  const int S = p.T;
  long long my_beg = 0, my_len = 0;
  if (lane < a.W && i0 + lane < a.R) {
    const int64_t r = a.row_order ? a.row_order[i0 + lane] : i0 + lane;
    if (r >= 0 && r < a.R) {
      const int64_t beg = clampi(a.indptr[r], 0, a.nnz);
      const int64_t end = clampi(a.indptr[r + 1], beg, a.nnz);
      my_beg = beg;
      my_len = end - beg;
      if (a.G > 0 && my_len > kChunk) my_len = 0;  // the pieces' launches take it
    }
  }
  long long maxlen = my_len;
  for (int o = 1; o < 64; o <<= 1) {
    const long long t = __shfl_xor(maxlen, o);
    maxlen = t > maxlen ? t : maxlen;
  }
  if (maxlen == 0) return;
  // the team: the power of two that covers the longest row, at most the wave
  int T = 1;
  while (T < S && T < maxlen) T <<= 1;
  const int P = S / T;  // rows side by side
  const int64_t nsteps = (maxlen + T - 1) / T;
  const int team = p.q / T;
  p.q = p.q - team * T;
  p.T = T;
  for (int b = 0; b < a.W; b += P) {
    const int i = b + team;  // < 64: W <= S, and P > W only in a single batch
    const int64_t beg = __shfl(my_beg, i);
    const int64_t len = __shfl(my_len, i);
    team_range<V, BWD, false>(a, p, beg, len, nsteps, nullptr, nullptr);
  }
}

// The piece of a long row in block g = item / 2: the row that holds the
// block's first slot (item even) or the one that starts inside the block
// (odd). Slots [k0, k1) of row r; `first` is the workspace slot of the row's
// first piece, where the combined result is left. The same in every lane.
__device__ __forceinline__ bool piece_of(const Args& a, int64_t item, int lane, int64_t& k0,
                                         int64_t& k1, int64_t& first) {
  const int64_t g = item >> 1;
  const bool inner = item & 1;
  const int64_t b0 = g * kChunk;
  if (g >= a.G || b0 >= a.nnz) return false;
  const int64_t b1 = b0 + kChunk < a.nnz ? b0 + kChunk : a.nnz;
  const int64_t r = row_of(a.indptr, a.R, inner ? b1 - 1 : b0, lane);
  if (r >= a.R) return false;
  const int64_t beg = clampi(a.indptr[r], 0, a.nnz);
  const int64_t end = clampi(a.indptr[r + 1], beg, a.nnz);
  if (end - beg <= kChunk) return false;
  if (inner ? beg <= b0 : beg > b0) return false;
  k0 = beg > b0 ? beg : b0;
  k1 = end < b1 ? end : b1;
  const int64_t g0 = beg / kChunk;
  first = 2 * g0 + (beg > g0 * kChunk ? 1 : 0);
  return k0 < k1;
}

// A piece is a workgroup's, a quarter of the block's slots per wave, so at
// H <= 16 (V = 4) the piece is read once, into registers.
template <int V, bool BWD>
__global__ __launch_bounds__(kThreads) void edge_softmax_piece_kernel(Args a) {
  __shared__ float sm[kWaves * 64 * V];
  const int64_t item = block_linear() / a.tiles, tile = block_linear() - item * a.tiles;
  const int lane = threadIdx.x & 63;
  int64_t k0, k1, first;
  if (!piece_of(a, item, lane, k0, k1, first)) return;  // the whole workgroup
  const Place p = place_of<V>(a, tile, lane);
  constexpr int64_t Q = kChunk / kWaves;
  const int64_t beg = k0 + (threadIdx.x >> 6) * Q;
  const int64_t len = beg >= k1 ? 0 : (k1 - beg < Q ? k1 - beg : Q);
  team_range<V, BWD, true>(a, p, beg, len, (Q + p.T - 1) / p.T, a.partial + item * 2 * a.H, sm);
}

// One thread per (row, column): the pieces of a long row in block order.
template <bool BWD>
__global__ __launch_bounds__(kThreads) void edge_softmax_combine_kernel(Args a) {
  const int64_t i = block_linear() * kThreads + threadIdx.x;
  if (i >= a.R * a.H) return;
  const int64_t r = i / a.H, c = i - r * a.H;
  const int64_t beg = clampi(a.indptr[r], 0, a.nnz);
  const int64_t end = clampi(a.indptr[r + 1], beg, a.nnz);
  if (end - beg <= kChunk) return;
  const int64_t g0 = beg / kChunk, g1 = (end - 1) / kChunk;
  const int64_t first = 2 * g0 + (beg > g0 * kChunk ? 1 : 0);
  const int64_t PW = 2 * a.H;
  float* res = a.partial + first * PW + 2 * c;
  if constexpr (BWD) {
    float t = res[0];
    for (int64_t g = g0 + 1; g <= g1; ++g) t = t + a.partial[2 * g * PW + 2 * c];
    res[0] = t;
  } else {
    float m = res[0];
    for (int64_t g = g0 + 1; g <= g1; ++g) m = nanmax(m, a.partial[2 * g * PW + 2 * c]);
    // a piece of only -inf beside a larger maximum adds nothing (its own sum
    // is NaN: -inf - -inf); when every piece is one, m is -inf and the
    // stores' x - m is NaN
    float s = 0.0f;
    for (int64_t g = g0; g <= g1; ++g) {
      const float* q = g == g0 ? res : a.partial + 2 * g * PW + 2 * c;
      if (q[0] != -INFINITY) s = s + q[1] * expf(q[0] - m);
    }
    res[0] = m;
    res[1] = s;
  }
}

template <int V, bool BWD>
__global__ __launch_bounds__(kThreads) void edge_softmax_finish_kernel(Args a) {
  const int64_t item = block_linear() / a.tiles, tile = block_linear() - item * a.tiles;
  const int lane = threadIdx.x & 63;
  int64_t k0, k1, first;
  if (!piece_of(a, item, lane, k0, k1, first)) return;
  const Place p = place_of<V>(a, tile, lane);
  if (!p.colok) return;
  const float* res = a.partial + first * 2 * a.H + 2 * p.col0;
  float m[V], s[V];
#pragma unroll
  for (int c = 0; c < V; ++c) {
    m[c] = res[2 * c];
    s[c] = res[2 * c + 1];
  }
#pragma unroll 4
  for (int64_t k = k0 + (threadIdx.x >> 6) * p.T + p.q; k < k1; k += kWaves * p.T) {
    const int64_t off = slot_offset(a, k) + p.col0;
    float v[V], o[V];
    load_cols<V>(a.x + off, v);
    if constexpr (BWD) {
      float g[V];
      load_cols<V>(a.dy + off, g);
#pragma unroll
      for (int c = 0; c < V; ++c) o[c] = v[c] * (g[c] - m[c]);
    } else {
#pragma unroll
      for (int c = 0; c < V; ++c) o[c] = expf(v[c] - m[c]) / s[c];
    }
    store_cols<V>(a.out + off, o);
  }
}

int lanes_shift(int64_t H, int V) {
  const int64_t need = (H + V - 1) / V;
  int sh = 0;
  while (sh < 6 && (int64_t(1) << sh) < need) ++sh;
  return sh;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int64_t num_blocks(int64_t nnz) { return (nnz + kChunk - 1) / kChunk; }

template <bool BWD>
void launch(int64_t R, int64_t nnz, int64_t H, const int64_t* indptr, const int64_t* eid,
            const int32_t* row_order, const float* x, const float* dy, float* out,
            int64_t max_row_len, void* workspace, hipStream_t stream) {
  DGLHIP_CHECK(R >= 0 && nnz >= 0 && H >= 0, "negative size");
  if (R == 0 || nnz == 0 || H == 0) return;
  DGLHIP_CHECK(indptr && x && out && (!BWD || dy), "null pointer argument");
  const bool pieces = nnz > kChunk && (max_row_len < 0 || max_row_len > kChunk);
  DGLHIP_CHECK(!pieces || workspace, "rows longer than a chunk need the workspace");
  Args a;
  a.R = R; a.nnz = nnz; a.H = H;
  a.G = pieces ? num_blocks(nnz) : 0;
  a.indptr = indptr; a.eid = eid; a.row_order = row_order;
  a.x = x; a.dy = dy; a.out = out;
  a.partial = static_cast<float*>(workspace);
  // 16-byte accesses where every slot's columns allow them
  const bool vec = H % 4 == 0 && aligned16(x) && aligned16(out) && (!BWD || aligned16(dy));
  const int V = vec ? 4 : 1;
  a.lps_shift = lanes_shift(H, V);
  const int64_t lps = int64_t(1) << a.lps_shift, S = 64 / lps;
  a.tiles = (H + lps * V - 1) / (lps * V);
  // rows per wave: as many as fill its registers at the mean row length
  const int64_t mean = nnz / R > 1 ? nnz / R : 1;
  a.W = 1;
  while (a.W * 2 <= S && a.W * 2 * mean <= S * kRegSteps<BWD>) a.W *= 2;
  const dim3 rgrid = grid_1d(((R + a.W - 1) / a.W * a.tiles + kWaves - 1) / kWaves);
  if (vec)
    hipLaunchKernelGGL((edge_softmax_rows_kernel<4, BWD>), rgrid, dim3(kThreads), 0, stream, a);
  else
    hipLaunchKernelGGL((edge_softmax_rows_kernel<1, BWD>), rgrid, dim3(kThreads), 0, stream, a);
  DGLHIP_CHECK(hipGetLastError() == hipSuccess, "edge softmax launch failed");
  if (!pieces) return;
  const dim3 pgrid = grid_1d(2 * a.G * a.tiles);
  const dim3 cgrid = grid_1d((R * H + kThreads - 1) / kThreads);
  if (vec)
    hipLaunchKernelGGL((edge_softmax_piece_kernel<4, BWD>), pgrid, dim3(kThreads), 0, stream, a);
  else
    hipLaunchKernelGGL((edge_softmax_piece_kernel<1, BWD>), pgrid, dim3(kThreads), 0, stream, a);
  hipLaunchKernelGGL((edge_softmax_combine_kernel<BWD>), cgrid, dim3(kThreads), 0, stream, a);
  if (vec)
    hipLaunchKernelGGL((edge_softmax_finish_kernel<4, BWD>), pgrid, dim3(kThreads), 0, stream, a);
  else
    hipLaunchKernelGGL((edge_softmax_finish_kernel<1, BWD>), pgrid, dim3(kThreads), 0, stream, a);
  DGLHIP_CHECK(hipGetLastError() == hipSuccess, "edge softmax piece launch failed");
}

}  // namespace

}  // namespace dglhip

using namespace dglhip;

extern "C" {

int64_t dglhip_edge_softmax_workspace_bytes(int64_t num_rows, int64_t nnz, int64_t feat_len) {
  if (nnz <= kChunk || num_rows <= 0 || feat_len <= 0) return 0;
  return 2 * num_blocks(nnz) * 2 * feat_len * 4;
}

int dglhip_edge_softmax_device(int64_t num_rows, int64_t nnz, int64_t feat_len,
                               const int64_t* indptr, const int64_t* eid,
                               const int32_t* row_order, const float* x, float* y,
                               int64_t max_row_len, void* workspace, void* stream) {
  API_BEGIN();
  launch<false>(num_rows, nnz, feat_len, indptr, eid, row_order, x, nullptr, y, max_row_len,
                workspace, static_cast<hipStream_t>(stream));
  API_END();
}

int dglhip_edge_softmax_bwd_device(int64_t num_rows, int64_t nnz, int64_t feat_len,
                                   const int64_t* indptr, const int64_t* eid,
                                   const int32_t* row_order, const float* y, const float* dy,
                                   float* dx, int64_t max_row_len, void* workspace,
                                   void* stream) {
  API_BEGIN();
  launch<true>(num_rows, nnz, feat_len, indptr, eid, row_order, y, dy, dx, max_row_len,
               workspace, static_cast<hipStream_t>(stream));
  API_END();
}

}  // extern "C"
