// Segment reduction over consecutive row ranges: the readout of a batched
// graph (sum / mean / max of each graph's node or edge rows) and its backward.
//
// y[s, :] = REDUCE over rows [offsets[s], offsets[s+1]) of x (optionally
// w[i] * x[i, :]), as one sequential float32 chain per column in row order
// from +0.0f: the bits of torch's CPU scatter_add_. A segment longer than
// DGLHIP_SEGMENT_CHUNK rows is cut into chunks of that many rows from its
// start, each chunk a chain from zero, the chunk sums added in chunk order.
//
// Mapping. A lane owns V columns (V = 4 with 16-byte loads when F % 4 == 0 and
// the rows are 16-byte aligned, else 1) and walks its rows in order, so the
// lanes of a group read consecutive columns of one row. A group is LPS =
// min(64, pow2 >= F / V) lanes; a wave holds 64 / LPS groups, each on its own
// item, so small F packs several segments into one wave; F > 64 V columns are
// tiled over waves. Loads run kAhead rows in front of the adds (the add order
// is the chain's, the load order is free).
//
// Items, from the sizes alone (no host sync, no data-dependent geometry):
// item s < B is the first chunk of segment s; item B + g belongs to the block
// of rows [g C, (g + 1) C). Later chunks of long segments start at least C
// rows apart, so a block holds the start of at most one, and it is a chunk of
// the segment that contains row g C: the item finds that segment by a binary
// search of the offsets, and writes the chunk's partial to slot g of the
// workspace. A second launch adds each long segment's partials in order. A
// caller that knows the longest segment (host-side sizes) passes it, and both
// the block items and the second launch are skipped when it is <= C.
//
// No atomics; every output element is written exactly once.
#include "../../include/dgl_hip.h"
#include "common.h"
#include "launch.h"

#include <hip/hip_runtime.h>

namespace dglhip {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int64_t kChunk = DGLHIP_SEGMENT_CHUNK;
constexpr int64_t kFillWaves = 1024;  // 256 compute units x 4 SIMDs

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

// torch.max(x, 0) on the CPU: the first row attaining the maximum, or the
// first NaN
__device__ __forceinline__ void max_step(float v, int64_t r, float& best, int64_t& arg) {
  if (!(best != best) && (v > best || v != v)) {
    best = v;
    arg = r;
  }
}

struct FwdArgs {
  int64_t B, N, F, G;  // G block items (0: no segment is longer than a chunk)
  int64_t PW;          // floats per partial slot: F columns, the weight sum, 16-byte pad
  int64_t ldx;
  int lps_shift;  // log2 of the lanes per group
  int64_t tiles;  // column tiles per item
  int mean;
  const int64_t* offsets;
  const float* x;
  const float* w;
  float* y;
  float* wsum;
  int64_t* arg;
  float* partial;  // G x PW
  float* wpart0;   // B: a long segment's first chunk of the weight sum
  int64_t* parg;   // G x F
};

// rows loaded in front of the adds: 64 registers of loads per lane either way
template <int V>
constexpr int kAhead = V == 4 ? 16 : 32;

// One wave per workgroup: a launch of few waves (one huge segment is a few
// hundred chunks) then spreads over as many compute units as it has waves.
template <int V, bool MAX, bool HASW>
__global__ __launch_bounds__(64) void segment_fwd_kernel(FwdArgs a) {
#pragma clang fp contract(off)
  constexpr int A = kAhead<V>;
  const int64_t wave = block_linear();
  const int lane = threadIdx.x;
  const int lps = 1 << a.lps_shift;
  const int64_t group = wave / a.tiles, tile = wave - group * a.tiles;
  const int64_t item = group * (64 >> a.lps_shift) + (lane >> a.lps_shift);
  const int64_t col0 = (tile * lps + (lane & (lps - 1))) * V;
  if (item >= a.B + a.G || col0 >= a.F) return;
  // rows [r0, r1) of segment s, written to y (first chunks) or to the slot
  int64_t s, r0, r1, len, slot = -1;
  if (item < a.B) {
    s = item;
    const int64_t beg = clampi(a.offsets[s], 0, a.N);
    const int64_t end = clampi(a.offsets[s + 1], beg, a.N);
    len = end - beg;
    r0 = beg;
    r1 = len > kChunk ? beg + kChunk : end;
  } else {
    const int64_t g = item - a.B, row0 = g * kChunk;
    s = segment_of(a.offsets, a.B, row0);
    if (s >= a.B) return;
    const int64_t beg = clampi(a.offsets[s], 0, a.N);
    const int64_t end = clampi(a.offsets[s + 1], beg, a.N);
    if (row0 < beg) return;
    const int64_t k = (row0 - beg + kChunk - 1) / kChunk;
    const int64_t p = beg + k * kChunk;
    if (k < 1 || p >= end || p >= row0 + kChunk) return;
    len = end - beg;
    r0 = p;
    r1 = p + kChunk < end ? p + kChunk : end;
    slot = g;
  }
  const float* xp = a.x + col0;
  float acc[V];
  int besti[V];  // max: the row of the maximum, relative to r0 (a chunk is 1024 rows)
  float wacc = 0.0f;
  const int n = static_cast<int>(r1 - r0);
#pragma unroll
  for (int k = 0; k < V; ++k) {
    acc[k] = 0.0f;
    besti[k] = -1;
  }
  int i = 0;
  if constexpr (MAX) {
    if (n > 0) {
      load_cols<V>(xp + r0 * a.ldx, acc);
#pragma unroll
      for (int k = 0; k < V; ++k) besti[k] = 0;
      i = 1;
    }
  }
  // batches of A rows: the loads of a batch are issued before its first add;
  // the rows past the end of the last batch re-read the last row and are not
  // added
  for (; i < n; i += A) {
    float v[A][V];
    float wv[A];
#pragma unroll
    for (int u = 0; u < A; ++u) {
      const int j = i + u < n ? i + u : n - 1;
      load_cols<V>(xp + (r0 + j) * a.ldx, v[u]);
      if constexpr (HASW) wv[u] = a.w[r0 + j];
    }
#pragma unroll
    for (int u = 0; u < A; ++u) {
      if (i + u < n) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
          if constexpr (MAX) {
            if (!(acc[k] != acc[k]) && (v[u][k] > acc[k] || v[u][k] != v[u][k])) {
              acc[k] = v[u][k];
              besti[k] = i + u;
            }
          } else if constexpr (HASW) {
            const float t = wv[u] * v[u][k];
            acc[k] = acc[k] + t;
          } else {
            acc[k] = acc[k] + v[u][k];
          }
        }
        if constexpr (HASW) wacc = wacc + wv[u];
      }
    }
  }
  int64_t best[V];
#pragma unroll
  for (int k = 0; k < V; ++k) best[k] = besti[k] < 0 ? -1 : r0 + besti[k];
  if (slot >= 0) {  // a later chunk's partial
    store_cols<V>(a.partial + slot * a.PW + col0, acc);
    if constexpr (MAX) {
#pragma unroll
      for (int k = 0; k < V; ++k) a.parg[slot * a.F + col0 + k] = best[k];
    }
    if (HASW && col0 == 0) a.partial[slot * a.PW + a.F] = wacc;
    return;
  }
  const bool is_long = len > kChunk && a.G > 0;
  if (!MAX && a.mean && !is_long) {
    const float d = HASW ? wacc : static_cast<float>(len > 1 ? len : 1);
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = acc[k] / d;
  }
  store_cols<V>(a.y + s * a.F + col0, acc);
  if constexpr (MAX) {
#pragma unroll
    for (int k = 0; k < V; ++k) a.arg[s * a.F + col0 + k] = best[k];
  }
  if (HASW && col0 == 0) {
    if (is_long) a.wpart0[s] = wacc;
    else if (a.wsum) a.wsum[s] = wacc;
  }
}

// The second launch: thread (s, c) of a segment of more than one chunk adds
// the partials of column c in chunk order to the first chunk's result in y;
// column F is the weight sum.
template <bool MAX, bool HASW>
__global__ __launch_bounds__(kThreads) void segment_combine_kernel(FwdArgs a) {
#pragma clang fp contract(off)
  const int64_t i = block_linear() * kThreads + threadIdx.x;
  const int64_t W = a.F + 1;
  if (i >= a.B * W) return;
  const int64_t s = i / W, c = i - s * W;
  const int64_t beg = clampi(a.offsets[s], 0, a.N);
  const int64_t end = clampi(a.offsets[s + 1], beg, a.N);
  const int64_t len = end - beg;
  if (len <= kChunk) return;
  const int64_t g1 = (beg + kChunk) / kChunk;  // the slot of chunk k is g1 + k - 1
  const int64_t nk = (len + kChunk - 1) / kChunk;
  float wtot = 0.0f;
  if constexpr (HASW) {
    wtot = a.wpart0[s];
    for (int64_t k = 1; k < nk; ++k) wtot = wtot + a.partial[(g1 + k - 1) * a.PW + a.F];
  }
  if (c == a.F) {
    if (HASW && a.wsum) a.wsum[s] = wtot;
    return;
  }
  float tot = a.y[s * a.F + c];
  if constexpr (MAX) {
    int64_t best = a.arg[s * a.F + c];
    for (int64_t k = 1; k < nk; ++k)
      max_step(a.partial[(g1 + k - 1) * a.PW + c], a.parg[(g1 + k - 1) * a.F + c], tot, best);
    a.arg[s * a.F + c] = best;
  } else {
    for (int64_t k = 1; k < nk; ++k) tot = tot + a.partial[(g1 + k - 1) * a.PW + c];
    if (a.mean) tot = tot / (HASW ? wtot : static_cast<float>(len));
  }
  a.y[s * a.F + c] = tot;
}

struct BwdArgs {
  int64_t B, N, F;
  int64_t ldx;
  int lps_shift;
  const int64_t* offsets;
  const float* dy;
  const float* x;
  const float* w;
  const float* y;
  const float* wsum;
  const int64_t* arg;
  float* dx;
  float* dw;
};

enum { kBwdSum = 0, kBwdMean = 1, kBwdWMean = 2, kBwdMax = 3 };

// One pass over the rows: a wave takes 64 consecutive rows, lane j finds the
// segment of row j (binary search), then the groups of LPS lanes walk the
// rows, each lane V columns at a time. dx rows are written whole; dw[i] is the
// group's sum of the lanes' dots.
template <int V, int MODE>
__global__ __launch_bounds__(kThreads) void segment_bwd_kernel(BwdArgs a) {
#pragma clang fp contract(off)
  const int64_t wave = block_linear() * kWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int64_t row_base = wave * 64;
  if (row_base >= a.N) return;  // the whole wave
  int64_t my_seg = 0;
  if (row_base + lane < a.N) {
    my_seg = segment_of(a.offsets, a.B, row_base + lane);
    if (my_seg >= a.B) my_seg = a.B - 1;
  }
  const int lps = 1 << a.lps_shift, spw = 64 >> a.lps_shift;
  const int sub = lane >> a.lps_shift, l = lane & (lps - 1);
  for (int it = 0; it < lps; ++it) {
    const int rr = it * spw + sub;
    const int64_t s = __shfl(static_cast<int>(my_seg), rr);
    const int64_t row = row_base + rr;
    const bool live = row < a.N;
    float dot = 0.0f;
    if (live) {
      float wr = 1.0f, div = 1.0f;
      if (a.w) wr = a.w[row];
      if (MODE == kBwdMean) {
        const int64_t beg = clampi(a.offsets[s], 0, a.N);
        const int64_t end = clampi(a.offsets[s + 1], beg, a.N);
        div = static_cast<float>(end - beg > 1 ? end - beg : 1);
      } else if (MODE == kBwdWMean) {
        div = a.wsum[s];
      }
      for (int64_t c = int64_t(l) * V; c < a.F; c += int64_t(lps) * V) {
        float g[V], o[V];
        load_cols<V>(a.dy + s * a.F + c, g);
        if (MODE == kBwdMean || MODE == kBwdWMean) {
#pragma unroll
          for (int k = 0; k < V; ++k) g[k] = g[k] / div;
        }
        if (MODE == kBwdMax) {
#pragma unroll
          for (int k = 0; k < V; ++k) o[k] = a.arg[s * a.F + c + k] == row ? g[k] : 0.0f;
        } else {
#pragma unroll
          for (int k = 0; k < V; ++k) o[k] = a.w ? g[k] * wr : g[k];
        }
        store_cols<V>(a.dx + row * a.F + c, o);
        if (a.dw) {
          float xv[V];
          load_cols<V>(a.x + row * a.ldx + c, xv);
          if (MODE == kBwdWMean) {
            float yv[V];
            load_cols<V>(a.y + s * a.F + c, yv);
#pragma unroll
            for (int k = 0; k < V; ++k) xv[k] = xv[k] - yv[k];
          }
#pragma unroll
          for (int k = 0; k < V; ++k) dot += g[k] * xv[k];
        }
      }
    }
    if (a.dw) {  // every lane of the wave takes part in the shuffles
      for (int m = lps >> 1; m > 0; m >>= 1) dot += __shfl_xor(dot, m);
      if (live && l == 0) a.dw[row] = dot;
    }
  }
}

int lanes_shift(int64_t F, int V) {
  const int64_t need = (F + V - 1) / V;
  int sh = 0;
  while (sh < 6 && (int64_t(1) << sh) < need) ++sh;
  return sh;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int64_t block_items(int64_t N) { return (N + kChunk - 1) / kChunk; }

int64_t round8(int64_t v) { return (v + 7) & ~int64_t(7); }

int64_t partial_width(int64_t F) { return (F + 4) & ~int64_t(3); }

}  // namespace

}  // namespace dglhip

using namespace dglhip;

extern "C" {

int64_t dglhip_segment_reduce_workspace_bytes(int reduce_op, int64_t num_segments,
                                              int64_t num_rows, int64_t feat_len) {
  if (num_rows <= kChunk || num_segments <= 0 || feat_len <= 0) return 0;
  const int64_t G = block_items(num_rows);
  int64_t bytes = round8((G * partial_width(feat_len) + num_segments) * 4);
  if (reduce_op == DGLHIP_REDUCE_MAX) bytes += G * feat_len * 8;
  return bytes;
}

int dglhip_segment_reduce_device(int reduce_op, int64_t num_segments, int64_t num_rows,
                                 int64_t feat_len, const int64_t* offsets, const float* x,
                                 int64_t ldx, const float* weight, float* y, float* wsum,
                                 int64_t* arg, int64_t max_segment_rows, void* workspace,
                                 void* stream_) {
  API_BEGIN();
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  DGLHIP_CHECK(reduce_op == DGLHIP_REDUCE_SUM || reduce_op == DGLHIP_REDUCE_MAX ||
                   reduce_op == DGLHIP_REDUCE_MEAN,
               "unknown reduce op " << reduce_op);
  DGLHIP_CHECK(num_segments >= 0 && num_rows >= 0 && feat_len >= 0, "negative size");
  if (num_segments == 0 || feat_len == 0) return 0;
  const bool is_max = reduce_op == DGLHIP_REDUCE_MAX;
  const bool mean = reduce_op == DGLHIP_REDUCE_MEAN;
  DGLHIP_CHECK(!(is_max && weight), "the max reducer takes no weight");
  DGLHIP_CHECK(offsets && y && (num_rows == 0 || x), "null pointer argument");
  DGLHIP_CHECK(ldx >= feat_len, "row stride below the row width");
  DGLHIP_CHECK(!is_max || arg, "the max reducer needs arg");
  DGLHIP_CHECK(!(mean && weight) || wsum, "the weighted mean needs wsum");
  const bool chunks = num_rows > kChunk && (max_segment_rows < 0 || max_segment_rows > kChunk);
  DGLHIP_CHECK(!chunks || workspace, "segments longer than a chunk need the workspace");
  FwdArgs a;
  a.B = num_segments; a.N = num_rows; a.F = feat_len;
  a.G = chunks ? block_items(num_rows) : 0;
  a.PW = partial_width(feat_len);
  a.ldx = ldx;
  a.mean = mean ? 1 : 0;
  a.offsets = offsets; a.x = x; a.w = weight; a.y = y; a.wsum = wsum; a.arg = arg;
  a.partial = static_cast<float*>(workspace);
  a.wpart0 = a.partial ? a.partial + a.G * a.PW : nullptr;
  a.parg = a.partial ? reinterpret_cast<int64_t*>(static_cast<char*>(workspace) +
                                                  round8((a.G * a.PW + num_segments) * 4))
                     : nullptr;
  const int64_t items = a.B + a.G;
  auto waves_at = [&](int V) {
    a.lps_shift = lanes_shift(feat_len, V);
    const int64_t lps = int64_t(1) << a.lps_shift, spw = 64 / lps;
    a.tiles = (feat_len + lps * V - 1) / (lps * V);
    return (items + spw - 1) / spw * a.tiles;
  };
  // 16-byte loads where the rows allow them and they still leave a wave for
  // every SIMD (kFillWaves); below that, one column per lane makes up to four
  // times the waves, which a launch that cannot fill the chip needs more
  bool vec = feat_len % 4 == 0 && ldx % 4 == 0 && aligned16(x) && aligned16(y) &&
             (!a.partial || aligned16(a.partial));
  if (vec && waves_at(4) < kFillWaves) vec = false;
  const int64_t waves = waves_at(vec ? 4 : 1);
  const dim3 grid = grid_1d(waves);
#define DGLHIP_SEG_FWD(VV, MX, HW) \
  hipLaunchKernelGGL((segment_fwd_kernel<VV, MX, HW>), grid, dim3(64), 0, stream, a)
  if (is_max) {
    if (vec) DGLHIP_SEG_FWD(4, true, false); else DGLHIP_SEG_FWD(1, true, false);
  } else if (weight) {
    if (vec) DGLHIP_SEG_FWD(4, false, true); else DGLHIP_SEG_FWD(1, false, true);
  } else {
    if (vec) DGLHIP_SEG_FWD(4, false, false); else DGLHIP_SEG_FWD(1, false, false);
  }
#undef DGLHIP_SEG_FWD
  DGLHIP_CHECK(hipGetLastError() == hipSuccess, "segment reduce launch failed");
  if (chunks) {
    const dim3 cgrid = grid_1d((a.B * (a.F + 1) + kThreads - 1) / kThreads);
    if (is_max)
      hipLaunchKernelGGL((segment_combine_kernel<true, false>), cgrid, dim3(kThreads), 0, stream, a);
    else if (weight)
      hipLaunchKernelGGL((segment_combine_kernel<false, true>), cgrid, dim3(kThreads), 0, stream, a);
    else
      hipLaunchKernelGGL((segment_combine_kernel<false, false>), cgrid, dim3(kThreads), 0, stream,
                         a);
    DGLHIP_CHECK(hipGetLastError() == hipSuccess, "segment combine launch failed");
  }
  API_END();
}

int dglhip_segment_reduce_bwd_device(int reduce_op, int64_t num_segments, int64_t num_rows,
                                     int64_t feat_len, const int64_t* offsets, const float* dy,
                                     const float* x, int64_t ldx, const float* weight,
                                     const float* y, const float* wsum, const int64_t* arg,
                                     float* dx, float* dw, void* stream_) {
  API_BEGIN();
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  DGLHIP_CHECK(reduce_op == DGLHIP_REDUCE_SUM || reduce_op == DGLHIP_REDUCE_MAX ||
                   reduce_op == DGLHIP_REDUCE_MEAN,
               "unknown reduce op " << reduce_op);
  DGLHIP_CHECK(num_segments >= 0 && num_rows >= 0 && feat_len >= 0, "negative size");
  if (num_rows == 0 || feat_len == 0) return 0;
  DGLHIP_CHECK(num_segments >= 1, "rows without a segment");
  const bool is_max = reduce_op == DGLHIP_REDUCE_MAX;
  const bool wmean = reduce_op == DGLHIP_REDUCE_MEAN && weight;
  DGLHIP_CHECK(!(is_max && weight), "the max reducer takes no weight");
  DGLHIP_CHECK(offsets && dy && dx, "null pointer argument");
  DGLHIP_CHECK(!is_max || arg, "the max reducer needs arg");
  DGLHIP_CHECK(!wmean || (wsum && (!dw || y)), "the weighted mean needs wsum and y");
  DGLHIP_CHECK(!dw || (weight && x && ldx >= feat_len), "dw needs weight and x");
  BwdArgs a;
  a.B = num_segments; a.N = num_rows; a.F = feat_len; a.ldx = ldx;
  a.offsets = offsets; a.dy = dy; a.x = x; a.w = weight; a.y = y; a.wsum = wsum; a.arg = arg;
  a.dx = dx; a.dw = dw;
  const bool vec = feat_len % 4 == 0 && aligned16(dy) && aligned16(dx) &&
                   (!dw || (ldx % 4 == 0 && aligned16(x) && (!wmean || aligned16(y))));
  const int V = vec ? 4 : 1;
  a.lps_shift = lanes_shift(feat_len, V);
  const int64_t waves = (num_rows + 63) / 64;
  const dim3 grid = grid_1d((waves + kWaves - 1) / kWaves);
  const int mode = is_max ? kBwdMax
                          : (reduce_op == DGLHIP_REDUCE_SUM ? kBwdSum
                                                            : (weight ? kBwdWMean : kBwdMean));
#define DGLHIP_SEG_BWD(M)                                                                      \
  do {                                                                                         \
    if (vec) hipLaunchKernelGGL((segment_bwd_kernel<4, M>), grid, dim3(kThreads), 0, stream, a); \
    else hipLaunchKernelGGL((segment_bwd_kernel<1, M>), grid, dim3(kThreads), 0, stream, a);   \
  } while (0)
  if (mode == kBwdSum) DGLHIP_SEG_BWD(kBwdSum);
  else if (mode == kBwdMean) DGLHIP_SEG_BWD(kBwdMean);
  else if (mode == kBwdWMean) DGLHIP_SEG_BWD(kBwdWMean);
  else DGLHIP_SEG_BWD(kBwdMax);
#undef DGLHIP_SEG_BWD
  DGLHIP_CHECK(hipGetLastError() == hipSuccess, "segment reduce backward launch failed");
  API_END();
}

}  // extern "C"
