// Segment fixed-radius neighbours (ball query): for every query row i of
// segment s of q (M, D), the first k rows j of segment s of the points x (N, D),
// in row order, with squared Euclidean distance below r2. The grouping step of
// a PointNet++ set abstraction (q: the sampled centroids) and, with q = x, the
// builder behind dgl.radius_graph. The contract is in dgl_hip.h; the host twin
// is segment_radius_host.cc and computes the same bits.
//
// Distance. segment_fps's chain: s = +0.0; for c ascending: t = x_j[c] - q_i[c];
// s = fmaf(t, t, s). Membership is the threshold d < r2 on these bits (a NaN is
// outside), so the chain is explicit fmaf on both sides and no MFMA expansion
// n_i + n_j - 2 <x_i, x_j>, whose cancellation near r2 would make membership
// differ between host and device. Rows are zero-filled to the width of the
// instantiation: fmaf(0, 0, s) = s leaves the bits alone.
//
// Selection is no top-k: "the first k members in row order" is an ordered
// compaction with an early exit. No sorted list, no merge, no threshold.
//
// Items, from the query offsets alone (segment_knn.hip's scheme, no host
// sync): item s < B is the first 64-query tile of query segment s; item B + g
// is the later tile that starts in queries [64 g, 64 g + 64). Empty and absent
// tiles cost one early exit of the whole workgroup, before any barrier.
//
// Lanes. A workgroup of four waves owns 64 queries, wave w the queries 16 w ..;
// lane l is (query l & 15, stripe l >> 4). The query's coordinates stay in V
// float4 registers (V in {1, 2, 4}: D <= 4, 8, 16) for the whole walk.
//
// Candidates. The segment's rows pass through LDS in tiles of 256 rows of 4 V
// floats: lane t loads elements t + 256 i of the tile (row e / 4V, column e %
// 4V; consecutive lanes read consecutive floats of the rows) and stores them
// at xs[e], conflict-free. The next tile's loads are issued into registers
// before the current tile's compares. In step j a lane reads row 4 j + stripe:
// a wave reads four 16-byte addresses per ds_read_b128, each broadcast to 16
// lanes.
//
// Ordered append without atomics. Each step takes one ballot of the hit bits.
// The rows of a step ascend with the stripe, so a hit's slot is its query's
// running count plus the popcount of the hits of the query's lower stripes in
// that ballot; every one of the query's four lanes adds the popcount of all
// four and so keeps the same count. Hits with slot < k go to the query's list
// in LDS (row within the segment, distance). At the end each wave writes its
// queries' rows of nbr / dist with consecutive lanes on consecutive slots; the
// padding (-1 / +inf, or the first member with PAD_FIRST) is folded into that
// write.
//
// Early exit. A wave whose queries all hold k members (queries past the end of
// the tile count as full) sets done[w], and from then on skips the compares,
// never a barrier. A tile is: [read done] store tile, barrier A, prefetch,
// compares (the only place done[] is written), barrier B. The four flags are
// read only between barrier B of one tile and barrier A of the next, where no
// wave can write them: every wave reads the same four values, so the break is
// workgroup-uniform and no wave waits at a barrier another has left behind.
// Every return is either before the first barrier and taken by the whole
// workgroup (the item test) or after the last one.
//
// LDS: the stage 4 V KiB static, the lists 8 k bytes x 64 queries dynamic (at
// most 32 KiB), flags and counts 272 bytes. No global atomics, no allocation,
// offsets clamped to [0, rows].
#include "../../include/dgl_hip.h"
#include "common.h"
#include "launch.h"
#include "segment_items.h"

#include <hip/hip_runtime.h>

namespace dglhip {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kQueries = 64;  // query rows per workgroup
constexpr int kRows = 256;    // candidate rows per staged tile
static_assert(kQueries == 16 * kWaves, "a wave owns 16 queries");
static_assert(kRows % 4 == 0, "a step covers one row per stripe");

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct RadiusArgs {
  int64_t B, N, M;
  int D, k;
  float r2;
  int exclude_self, pad_first;
  int64_t ldx, ldq;
  const int64_t* x_offsets;
  const int64_t* q_offsets;
  const float* x;
  const float* q;
  int64_t* nbr;
  int32_t* cnt;
  float* dist;  // may be null
};

// V: float4s per row (D <= 4 V)
template <int V>
__global__ __launch_bounds__(kThreads) void segment_radius_kernel(RadiusArgs a) {
  constexpr int W = 4 * V;
  __shared__ __attribute__((aligned(16))) float xs[kRows * W];
  __shared__ int done[kWaves];
  __shared__ int cnts[kQueries];
  extern __shared__ __attribute__((aligned(16))) uint32_t lists[];
  uint32_t* ids = lists;  // [64][k]: the member's row within the segment
  float* ds = reinterpret_cast<float*>(lists + kQueries * a.k);  // [64][k]: its distance

  // the item: query tile q0 .. of query segment [qbeg, qend), candidate segment s
  const int64_t item = block_linear();
  int64_t s, qend, q0;
  if (item < a.B) {
    s = item;
    q0 = clampi(a.q_offsets[s], 0, a.M);
    qend = clampi(a.q_offsets[s + 1], q0, a.M);
  } else {
    const int64_t row0 = (item - a.B) * kQueries;
    if (row0 >= a.M) return;
    s = segment_of(a.q_offsets, a.B, row0);
    if (s >= a.B) return;
    const int64_t qbeg = clampi(a.q_offsets[s], 0, a.M);
    qend = clampi(a.q_offsets[s + 1], qbeg, a.M);
    if (row0 < qbeg) return;
    const int64_t tile = (row0 - qbeg + kQueries - 1) / kQueries;
    q0 = qbeg + tile * kQueries;
    if (tile < 1 || q0 >= qend || q0 >= row0 + kQueries) return;
  }
  if (q0 >= qend) return;  // a segment without queries; the whole workgroup, as above
  const int64_t xbeg = clampi(a.x_offsets[s], 0, a.N);
  const int len = static_cast<int>(clampi(a.x_offsets[s + 1], xbeg, a.N) - xbeg);
  const int nq = static_cast<int>(qend - q0 < kQueries ? qend - q0 : kQueries);

  const int t = threadIdx.x, w = t >> 6, lane = t & 63, h = lane >> 4;
  const int ql = 16 * w + (lane & 15);
  const bool on = ql < nq;
  const int k = a.k, D = a.D;
  const float r2 = a.r2;

  f32x4 qv[V];
  {
    const float* qr = a.q + (q0 + ql) * a.ldq;
#pragma unroll
    for (int c = 0; c < W; ++c) qv[c >> 2][c & 3] = (on && c < D) ? qr[c] : 0.0f;
  }
  // the candidate that is the query itself, as a row within the segment (-1: none)
  const int64_t self = a.exclude_self ? q0 + ql - xbeg : int64_t(-1);
  // the query's four lanes in a ballot, and those of the stripes below this one
  const uint64_t qmask = uint64_t(0x0001000100010001) << (lane & 15);
  const uint64_t lower = qmask & ((uint64_t(1) << lane) - 1);

  float sv[W];
  auto load_tile = [&](int c0) {
#pragma unroll
    for (int i = 0; i < W; ++i) {
      const int e = t + kThreads * i;
      const int col = e % W, row = c0 + e / W;
      sv[i] = (row < len && col < D) ? a.x[(xbeg + row) * a.ldx + col] : 0.0f;
    }
  };

  int count = 0;
  bool full = 16 * w >= nq;  // wave-uniform: no query of the wave wants a member
  if (lane == 0) done[w] = full;
  if (len > 0) load_tile(0);
  for (int c0 = 0; c0 < len; c0 += kRows) {
    // between barrier B of the last tile and barrier A of this one: nobody writes done[]
    if (c0 > 0 && (done[0] & done[1] & done[2] & done[3])) break;
#pragma unroll
    for (int i = 0; i < W; ++i) xs[t + kThreads * i] = sv[i];
    __syncthreads();  // A
    if (c0 + kRows < len) load_tile(c0 + kRows);
    if (!full) {
#pragma unroll 4
      for (int j = 0; j < kRows / 4; ++j) {
        const int row = 4 * j + h;
        const f32x4* p = reinterpret_cast<const f32x4*>(xs + row * W);
        float d = 0.0f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const f32x4 c = p[v];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float e = c[u] - qv[v][u];
            d = fmaf(e, e, d);
          }
        }
        const int cl = c0 + row;  // the candidate's row within the segment
        const bool hit = on && cl < len && d < r2 && cl != self;
        const uint64_t hits = __builtin_amdgcn_ballot_w64(hit);
        if (hits == 0) continue;  // wave-uniform
        const int slot = count + __builtin_popcountll(hits & lower);
        if (hit && slot < k) {
          ids[ql * k + slot] = static_cast<uint32_t>(cl);
          ds[ql * k + slot] = d;
        }
        count += __builtin_popcountll(hits & qmask);
      }
      full = __builtin_amdgcn_ballot_w64(on && count < k) == 0;
      if (full && lane == 0) done[w] = 1;
    }
    __syncthreads();  // B
  }

  const int c = count < k ? count : k;
  if (on && h == 0) {
    cnts[ql] = c;
    a.cnt[q0 + ql] = c;
  }
  __syncthreads();  // the last barrier: the lists and counts of the wave's queries
  if (16 * w >= nq) return;
  // consecutive lanes on consecutive slots of the wave's rows of the outputs
  const int slots = (nq - 16 * w < 16 ? nq - 16 * w : 16) * k;
  const uint32_t* wi = ids + 16 * w * k;
  const float* wd = ds + 16 * w * k;
  const int64_t base = (q0 + 16 * w) * k;
  for (int e = lane; e < slots; e += 64) {
    const int qq = e / k, n = cnts[16 * w + qq];
    // past the members: nothing, or the first member again
    const int src = e - qq * k < n ? e : ((a.pad_first && n > 0) ? qq * k : -1);
    a.nbr[base + e] = src < 0 ? int64_t(-1) : xbeg + static_cast<int64_t>(wi[src]);
    if (a.dist != nullptr) a.dist[base + e] = src < 0 ? __uint_as_float(0x7f800000u) : wd[src];
  }
}

template <int V>
void launch_radius(const RadiusArgs& a, hipStream_t stream) {
  const dim3 grid = grid_1d(a.B + (a.M + kQueries - 1) / kQueries);
  const size_t lists = size_t(kQueries) * a.k * (sizeof(uint32_t) + sizeof(float));
  hipLaunchKernelGGL(segment_radius_kernel<V>, grid, dim3(kThreads), lists, stream, a);
}

}  // namespace

}  // namespace dglhip

using namespace dglhip;

extern "C" {

int64_t dglhip_segment_radius_workspace_bytes(int64_t num_segments, int64_t num_rows,
                                              int64_t num_queries, int64_t dim, int64_t k) {
  (void)num_segments; (void)num_rows; (void)num_queries; (void)dim; (void)k;
  return 0;  // the lists live in LDS
}

int dglhip_segment_radius_device(int64_t num_segments, int64_t num_rows, int64_t num_queries,
                                 int64_t dim, int64_t k, float r2, int flags,
                                 const int64_t* x_offsets, const float* x, int64_t ldx,
                                 const int64_t* q_offsets, const float* q, int64_t ldq,
                                 int64_t* nbr, int32_t* cnt, float* dist, void* workspace,
                                 void* stream_) {
  API_BEGIN();
  (void)workspace;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  DGLHIP_CHECK(num_segments >= 0 && num_rows >= 0 && num_queries >= 0, "negative size");
  DGLHIP_CHECK(k >= 1 && k <= DGLHIP_RADIUS_MAX_K,
               "k = " << k << " outside [1, DGLHIP_RADIUS_MAX_K = " << DGLHIP_RADIUS_MAX_K << "]");
  DGLHIP_CHECK(dim >= 1 && dim <= DGLHIP_RADIUS_MAX_DIM,
               "D = " << dim << " outside [1, DGLHIP_RADIUS_MAX_DIM = " << DGLHIP_RADIUS_MAX_DIM
                      << "]");
  DGLHIP_CHECK(num_rows < (int64_t(1) << 31) && num_queries < (int64_t(1) << 31),
               "num_rows and num_queries must be below 2^31");
  DGLHIP_CHECK((flags & ~(DGLHIP_RADIUS_EXCLUDE_SELF | DGLHIP_RADIUS_PAD_FIRST)) == 0,
               "unknown flags " << flags);
  if (num_segments == 0 || num_queries == 0) return 0;
  DGLHIP_CHECK(x_offsets && q_offsets && q && nbr && cnt && (num_rows == 0 || x),
               "null pointer argument");
  DGLHIP_CHECK(ldx >= dim && ldq >= dim, "row stride below the row width");
  RadiusArgs a;
  a.B = num_segments; a.N = num_rows; a.M = num_queries;
  a.D = static_cast<int>(dim); a.k = static_cast<int>(k);
  a.r2 = r2;
  a.exclude_self = (flags & DGLHIP_RADIUS_EXCLUDE_SELF) ? 1 : 0;
  a.pad_first = (flags & DGLHIP_RADIUS_PAD_FIRST) ? 1 : 0;
  a.ldx = ldx; a.ldq = ldq;
  a.x_offsets = x_offsets; a.q_offsets = q_offsets; a.x = x; a.q = q;
  a.nbr = nbr; a.cnt = cnt; a.dist = dist;
  if (dim <= 4) launch_radius<1>(a, stream);
  else if (dim <= 8) launch_radius<2>(a, stream);
  else launch_radius<4>(a, stream);
  DGLHIP_CHECK(hipGetLastError() == hipSuccess, "segment radius launch failed");
  API_END();
}

}  // extern "C"
