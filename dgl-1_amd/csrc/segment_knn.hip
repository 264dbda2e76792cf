// Segment k-nearest neighbours on the f32 MFMA (v_mfma_f32_16x16x4_f32): for
// every row i of segment s of the points x (N, D), the k rows j of the same
// segment with the smallest squared Euclidean distance, as global row ids
// nbr (N, k) and distances dist (N, k), ascending. The builder behind
// dgl.knn_graph / segmented_knn_graph (DGCNN's dynamic graphs); no distance
// matrix is ever written.
//
// Distance. d(i, j) = n_i + n_j - 2 <x_i, x_j> in float32 with n_i = <x_i, x_i>
// (a pre-pass kernel, one fma chain per row), values that are not above zero
// set to +0.0 (a NaN stays NaN), d(i, i) = +0.0 by definition; with
// exclude_self the pair (i, i) is no candidate. The dot products are MFMA
// chains over D, zero-filled to the K steps of the instantiation.
//
// Order. A candidate is the packed word bits(d) << 32 | row within the segment
// (a NaN distance is keyed, and written, as 0x7fc00000: after +inf). d >= +0.0,
// so the unsigned order of the words is (d, j): an ascending stable sort. The
// order is strict: the result does not depend on how candidates reach a list.
// A slot without a candidate is the word ~0: index -1, distance +inf.
//
// Mapping. A workgroup of four waves owns a tile of 64 query rows of one
// segment, wave w the queries 16w .. 16w + 15. Items, from the offsets alone
// (no host sync; segment_topk.hip's scheme): item s < B is the first tile of
// segment s; item B + g is the later tile that starts in rows [64 g, 64 g + 64)
// (at most one: of the segment that contains row 64 g, found by a binary
// search). Unequal and empty segments cost one early exit each.
//
// A operands: lane l keeps x[query l & 15][4 s + (l >> 4)] for every K step s
// in KS registers for the whole kernel (node_linear.hip's map). The workgroup
// walks the segment's rows in candidate tiles of 64, each staged through LDS
// in K tiles of kCols = 4 min(KS, 8) columns as typed_linear_msg_kernel stages
// its source rows: coalesced row segments into xs[64][kCols + 2] (the 32 lanes
// of a half-wave read banks (kCols + 2)(l & 15) + (l >> 4): distinct, as
// (kCols + 2) / 2 is odd), the next K tile in registers before the current
// tile's MFMAs; the candidates' norms ride with the first K tile. B[k][col] =
// xs[16 t + col][k]: after the K loop accumulator i of column tile t is
// <x_q, x_c> for query 16w + 4(l >> 4) + i and candidate 16 t + (l & 15).
//
// Selection. Per query LDS holds a sorted list of LK words (KP = k rounded up
// to a power of two of them in use), the list's k-th word (the threshold) and
// a pending buffer of kPend = 32 words with a counter. A lane turns its 4 x 4
// accumulators into words in registers and appends the ones below the query's
// threshold through an LDS atomic on the counter. A column tile adds at most
// 16 words to a query, so the wave merges after a column tile that left some
// counter above 16, and once at the end. A merge is the wave's own (its 16
// queries are no other wave's: no workgroup barrier): the pending words are
// sorted by a 32-lane bitonic network of shuffles, c[i] = min(list[i],
// pending[KP - 1 - i]) is bitonic and holds the KP smallest, and log2 KP
// shuffle steps sort it. The threshold tightens with every merge, so after
// the first tiles hardly a word leaves the registers.
//
// LDS at LK = 64: lists 32 KiB + pending 16 KiB + stage 8.5 KiB + counters,
// thresholds, norms 1 KiB = 57.5 KiB static; LK = 32 (k <= 32): 41.5 KiB.
// No global atomics, no allocation, offsets clamped to [0, N].
#include "../../include/dgl_hip.h"
#include "common.h"
#include "launch.h"

#include <hip/hip_runtime.h>

namespace dglhip {

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 64;    // query rows per workgroup, candidate rows per tile
constexpr int kPend = 32;    // pending words per query
constexpr int kFlush = 16;   // a column tile's words per query at most
constexpr uint64_t kAbsent = ~uint64_t(0);
constexpr uint32_t kNaNBits = 0x7fc00000u;
static_assert(kPend - kFlush >= kFlush, "a column tile must fit after a skipped merge");

typedef float f32x4 __attribute__((ext_vector_type(4)));

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

// LDS traffic between the lanes of one wave: the wave's own program order
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
  const uint32_t lo = __shfl(static_cast<uint32_t>(v), src, 64);
  const uint32_t hi = __shfl(static_cast<uint32_t>(v >> 32), src, 64);
  return (uint64_t(hi) << 32) | lo;
}

__device__ __forceinline__ uint64_t min64(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t max64(uint64_t a, uint64_t b) { return a < b ? b : a; }

struct KnnArgs {
  int64_t B, N;
  int D, k, KP;  // KP: k rounded up to a power of two
  int exclude_self;
  int64_t ldx;
  const int64_t* offsets;
  const float* x;
  const float* norms;  // the workspace: n_i
  int64_t* nbr;
  float* dist;
};

__global__ __launch_bounds__(kThreads) void segment_knn_norms_kernel(int64_t N, int D, int64_t ldx,
                                                                     const float* __restrict__ x,
                                                                     float* __restrict__ norms) {
  const int64_t i = block_linear() * kThreads + threadIdx.x;
  if (i >= N) return;
  const float* p = x + i * ldx;
  float s = 0.0f;
  for (int c = 0; c < D; ++c) s = fmaf(p[c], p[c], s);
  norms[i] = s;
}

// Merge the c <= kPend pending words P of one query into its sorted list L
// (KP words in use), by the whole wave; the k-th word becomes the threshold.
__device__ __forceinline__ void merge_query(uint64_t* L, const uint64_t* P, int c, int KP, int k,
                                            uint64_t* thr, int lane) {
  uint64_t p = lane < c ? P[lane] : kAbsent;
  // ascending over lanes 0 .. 31 (the upper lanes hold kAbsent throughout)
#pragma unroll
  for (int kk = 2; kk <= kPend; kk <<= 1) {
#pragma unroll
    for (int j = kk >> 1; j > 0; j >>= 1) {
      const uint64_t o = shfl64(p, lane ^ j);
      const bool keep_min = ((lane & j) == 0) == ((lane & kk) == 0);
      p = keep_min ? min64(p, o) : max64(p, o);
    }
  }
  const int src = KP - 1 - lane;
  uint64_t pr = shfl64(p, src & 63);
  if (src < 0 || src >= kPend) pr = kAbsent;
  uint64_t v = lane < KP ? min64(L[lane], pr) : kAbsent;
  for (int j = KP >> 1; j > 0; j >>= 1) {
    const uint64_t o = shfl64(v, lane ^ j);
    v = (lane & j) == 0 ? min64(v, o) : max64(v, o);
  }
  if (lane < KP) L[lane] = v;
  if (lane == k - 1) *thr = v;
}

// KS: K steps of 4 held as A operands (D <= 4 KS); LK: list words per query
template <int KS, int LK>
__global__ __launch_bounds__(kThreads) void segment_knn_kernel(KnnArgs a) {
  constexpr int KT = KS < 8 ? KS : 8;  // K steps per staged tile
  constexpr int NKT = KS / KT;         // staged tiles per candidate tile
  constexpr int kCols = 4 * KT;
  constexpr int kSA = kCols + 2;
  constexpr int SQ = kTile * kCols / kThreads;  // staged values per lane: KT
  static_assert(KS % KT == 0 && SQ == KT, "the stage covers the tile exactly");
  __shared__ uint64_t list[kTile * LK];
  __shared__ uint64_t pend[kTile * kPend];
  __shared__ uint64_t thr[kTile];
  __shared__ int cnt[kTile];
  __shared__ float xs[kTile * kSA];
  __shared__ float ncs[kTile];

  // the item: query tile q0 .. of segment [beg, end)
  const int64_t item = block_linear();
  int64_t beg, end, q0;
  if (item < a.B) {
    beg = clampi(a.offsets[item], 0, a.N);
    end = clampi(a.offsets[item + 1], beg, a.N);
    q0 = beg;
  } else {
    const int64_t row0 = (item - a.B) * kTile;
    if (row0 >= a.N) return;
    const int64_t s = segment_of(a.offsets, a.B, row0);
    if (s >= a.B) return;
    beg = clampi(a.offsets[s], 0, a.N);
    end = clampi(a.offsets[s + 1], beg, a.N);
    if (row0 < beg) return;
    const int64_t q = (row0 - beg + kTile - 1) / kTile;
    q0 = beg + q * kTile;
    if (q < 1 || q0 >= end || q0 >= row0 + kTile) return;
  }
  if (q0 >= end) return;  // an empty segment; the whole workgroup, as above
  const int64_t len = end - beg;
  const int nq = static_cast<int>(end - q0 < kTile ? end - q0 : kTile);
  const int qoff = static_cast<int>(q0 - beg);  // first query's row within the segment

  const int t = threadIdx.x, w = t >> 6, lane = t & 63, r = lane & 15, h = lane >> 4;
  const bool busy = 16 * w < nq;  // wave-uniform: the wave owns a query
  const int k = a.k, KP = a.KP, D = a.D;

  // the wave's own lists, thresholds and counters
  for (int e = lane; e < 16 * LK; e += 64) list[16 * w * LK + e] = kAbsent;
  if (lane < 16) {
    thr[16 * w + lane] = kAbsent;
    cnt[16 * w + lane] = 0;
  }

  // A operands and the queries' norms
  float av[KS];
  {
    const bool on = 16 * w + r < nq;
    const float* xr = a.x + (q0 + 16 * w + r) * a.ldx;
#pragma unroll
    for (int s = 0; s < KS; ++s) av[s] = (on && 4 * s + h < D) ? xr[4 * s + h] : 0.0f;
  }
  float nqv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ql = 16 * w + 4 * h + i;
    nqv[i] = ql < nq ? a.norms[q0 + ql] : 0.0f;
  }

  // lane t stages element t + 256 q of a K tile: column e % kCols of candidate
  // row e / kCols; lanes 0 .. 63 the candidates' norms with the first K tile
  float sv[SQ], snorm = 0.0f;
  auto load_tile = [&](int64_t c0, int kt) {
#pragma unroll
    for (int q = 0; q < SQ; ++q) {
      const int e = t + kThreads * q;
      const int col = 4 * KT * kt + e % kCols;
      const int64_t row = c0 + e / kCols;
      sv[q] = (row < len && col < D) ? a.x[(beg + row) * a.ldx + col] : 0.0f;
    }
    if (kt == 0 && t < kTile) snorm = c0 + t < len ? a.norms[beg + c0 + t] : 0.0f;
  };
  auto store_tile = [&](int kt) {
#pragma unroll
    for (int q = 0; q < SQ; ++q) {
      const int e = t + kThreads * q;
      xs[(e / kCols) * kSA + e % kCols] = sv[q];
    }
    if (kt == 0 && t < kTile) ncs[t] = snorm;
  };

  uint64_t* wl = list + 16 * w * LK;
  uint64_t* wp = pend + 16 * w * kPend;
  // merge every query of the wave that has pending words
  auto merge_wave = [&]() {
    for (int q = 0; q < 16; ++q) {
      int c = __builtin_amdgcn_readfirstlane(cnt[16 * w + q]);
      if (c == 0) continue;
      if (c > kPend) c = kPend;
      merge_query(wl + q * LK, wp + q * kPend, c, KP, k, thr + 16 * w + q, lane);
      if (lane == 0) cnt[16 * w + q] = 0;
    }
    wave_sync();
  };

  load_tile(0, 0);
  for (int64_t c0 = 0; c0 < len; c0 += kTile) {
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float ncv[4];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      store_tile(kt);
      __syncthreads();
      if (kt + 1 < NKT) load_tile(c0, kt + 1);
      else if (c0 + kTile < len) load_tile(c0 + kTile, 0);
      if (kt == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) ncv[j] = ncs[16 * j + r];
      }
      if (busy) {
        const float* bp = xs + r * kSA + h;
#pragma unroll
        for (int s = 0; s < KT; ++s) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[KT * kt + s],
                                                          bp[16 * j * kSA + 4 * s], acc[j], 0, 0,
                                                          0);
        }
      }
      __syncthreads();
    }
    if (!busy) continue;
    // the filter, in registers: column tile j, query i of this lane
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t cl = c0 + 16 * j + r;  // candidate's row within the segment
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ql = 16 * w + 4 * h + i;
        if (ql >= nq || cl >= len) continue;
        const bool self = cl == qoff + ql;
        if (self && a.exclude_self) continue;
        const float v = (nqv[i] + ncv[j]) - 2.0f * acc[j][i];
        // not above zero: +0.0; a NaN stays one
        const float d = self ? 0.0f : (v > 0.0f ? v : (v == v ? 0.0f : v));
        const uint32_t bits = d == d ? __float_as_uint(d) : kNaNBits;
        const uint64_t word = (uint64_t(bits) << 32) | static_cast<uint32_t>(cl);
        if (word < thr[ql]) {
          const int slot = atomicAdd(&cnt[ql], 1);
          if (slot < kPend) pend[ql * kPend + slot] = word;
        }
      }
      wave_sync();
      const int c = lane < 16 ? cnt[16 * w + lane] : 0;
      if (__builtin_amdgcn_ballot_w64(c > kPend - kFlush) != 0) merge_wave();
    }
  }
  if (!busy) return;
  wave_sync();
  merge_wave();
  // lanes on consecutive slots of a query's row of the outputs
  for (int q = 0; q < 16; ++q) {
    const int ql = 16 * w + q;
    if (ql >= nq || lane >= k) continue;
    const uint64_t word = wl[q * LK + lane];
    const int64_t o = (q0 + ql) * k + lane;
    const bool none = word == kAbsent;
    a.nbr[o] = none ? int64_t(-1) : beg + static_cast<int64_t>(static_cast<uint32_t>(word));
    a.dist[o] = none ? __uint_as_float(0x7f800000u) : __uint_as_float(uint32_t(word >> 32));
  }
}

void check_sizes(int64_t B, int64_t N, int64_t D, int64_t k) {
  DGLHIP_CHECK(B >= 0 && N >= 0 && D >= 0, "negative size");
  DGLHIP_CHECK(k >= 1 && k <= DGLHIP_KNN_MAX_K,
               "k = " << k << " outside [1, DGLHIP_KNN_MAX_K = " << DGLHIP_KNN_MAX_K << "]");
  DGLHIP_CHECK(D <= DGLHIP_KNN_MAX_DIM,
               "D = " << D << " above DGLHIP_KNN_MAX_DIM = " << DGLHIP_KNN_MAX_DIM);
  DGLHIP_CHECK(N < (int64_t(1) << 31), "num_rows must be below 2^31");
}

template <int KS>
void launch_knn(const KnnArgs& a, hipStream_t stream) {
  const dim3 grid = grid_1d(a.B + (a.N + kTile - 1) / kTile);
  if (a.KP <= 32)
    hipLaunchKernelGGL((segment_knn_kernel<KS, 32>), grid, dim3(kThreads), 0, stream, a);
  else
    hipLaunchKernelGGL((segment_knn_kernel<KS, 64>), grid, dim3(kThreads), 0, stream, a);
}

}  // namespace

}  // namespace dglhip

using namespace dglhip;

extern "C" {

int64_t dglhip_segment_knn_workspace_bytes(int64_t num_segments, int64_t num_rows, int64_t dim,
                                           int64_t k) {
  (void)k;
  if (num_segments <= 0 || num_rows <= 0 || dim <= 0) return 0;
  return num_rows * 4;
}

int dglhip_segment_knn_device(int64_t num_segments, int64_t num_rows, int64_t dim, int64_t k,
                              int exclude_self, const int64_t* offsets, const float* x,
                              int64_t ldx, int64_t* nbr, float* dist, void* workspace,
                              void* stream_) {
  API_BEGIN();
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  check_sizes(num_segments, num_rows, dim, k);
  DGLHIP_CHECK(dim >= 1, "points without coordinates");
  if (num_segments == 0 || num_rows == 0) return 0;
  DGLHIP_CHECK(offsets && x && nbr && dist && workspace, "null pointer argument");
  DGLHIP_CHECK(ldx >= dim, "row stride below the row width");
  KnnArgs a;
  a.B = num_segments; a.N = num_rows;
  a.D = static_cast<int>(dim); a.k = static_cast<int>(k);
  a.KP = 1;
  while (a.KP < a.k) a.KP <<= 1;
  a.exclude_self = exclude_self ? 1 : 0;
  a.ldx = ldx; a.offsets = offsets; a.x = x;
  a.norms = static_cast<const float*>(workspace);
  a.nbr = nbr; a.dist = dist;
  hipLaunchKernelGGL(segment_knn_norms_kernel, grid_1d((num_rows + kThreads - 1) / kThreads),
                     dim3(kThreads), 0, stream, num_rows, a.D, ldx, x,
                     static_cast<float*>(workspace));
  DGLHIP_CHECK(hipGetLastError() == hipSuccess, "segment kNN norms launch failed");
  if (dim <= 4) launch_knn<1>(a, stream);
  else if (dim <= 16) launch_knn<4>(a, stream);
  else if (dim <= 64) launch_knn<16>(a, stream);
  else if (dim <= 128) launch_knn<32>(a, stream);
  else launch_knn<64>(a, stream);
  DGLHIP_CHECK(hipGetLastError() == hipSuccess, "segment kNN launch failed");
  API_END();
}

}  // extern "C"
