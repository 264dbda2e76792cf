// Segment farthest point sampling: m rows of every segment, each the row
// farthest from the rows picked before it (the sampler that opens every set
// abstraction of PointNet++). The contract is in dgl_hip.h; the host twin is
// segment_fps_host.cc and computes the same bits.
//
// The work is a chain: pick i needs pick i - 1, and a pick is one distance per
// row, a running minimum and an arg-max. What a call costs is the latency of
// one link times m, so a segment stays on one workgroup, on chip, for the
// whole call, and a link is built to be short.
//
// Key. The running minimum of a row is +0.0 .. +inf (the chain starts at +0.0
// and adds squares; a NaN distance never replaces it), so its bits order as
// unsigned integers. A row's key is (bits(mind) + 1) << 32 | ~row: the largest
// key is the largest mind and, among equals, the lowest row. A taken row keeps
// mind = -1.0f, which no distance is below, and its key's high word is 0; so
// does a lane's slot past the end of the segment. One unsigned 64-bit max is
// the whole pick rule, and it is strict: the result does not depend on how
// the rows are spread over lanes and waves.
//
// Link. A lane relaxes its RPL rows against the last pick and folds their keys;
// a wave reduces the keys over its rows of 16 lanes by DPP (xor 1, xor 2, half
// mirror, mirror) and over the four rows by v_readlane, which leaves the
// wave's key in scalar registers. Waves exchange keys through slots[pick & 1]
// in LDS: lane 0 of a wave stores, one __syncthreads(), then every wave loads
// all slots (lane l slot l & 15) and reduces them itself, again by DPP. The
// slot array is double-buffered, so a wave that runs ahead into pick i + 1
// writes the other half, and it cannot reach pick i + 2 before every wave has
// passed the barrier of pick i + 1, that is, has read the slots of pick i:
// one barrier per pick. A workgroup of one wave has no barrier at all. The
// winner's coordinates are then read by every lane from the segment's copy in
// LDS at a uniform address (a broadcast), not from memory.
//
// Residency, chosen on the host from the longest segment (max_segment_rows):
//  - resident, D <= 4 (kRegs): a lane holds its RPL rows' coordinates (padded
//    with zeros to 4, which leaves every chain's bits alone: fmaf(0, 0, s) is
//    s) and running minima in registers. The segment is staged once through
//    LDS, coalesced, and that copy (16 bytes a row) serves the winner reads.
//    After the staging no global memory is read.
//  - resident, D > 4: the segment is staged once in LDS with an odd row stride
//    (D | 1 floats: the lanes of a wave read one column of 64 different rows,
//    which an odd stride spreads over the banks); the running minima stay in
//    registers. It holds while rows x stride <= kLdsFloats (128 KiB of the
//    160 KiB of a gfx950 CU).
//  - general: any length, also when the sizes are known only on the device
//    (max_segment_rows < 0). 16 waves walk the segment's rows in memory every
//    pick (one cloud's rows stay in the L2; 16-byte loads where the rows
//    allow), the running minima live in the workspace, each touched by the
//    one lane that owns the row.
// (waves, RPL) of the resident kernels: 1 x 1, 1 x 4, 4 x 4, 16 x 4, 16 x 8 for
// segments of up to 64, 256, 1024, 4096 and 8192 rows.
//
// Output: one lane stores a pick as it is known; the stores are off the chain.
#include "../../include/dgl_hip.h"
#include "common.h"
#include "launch.h"

#include <hip/hip_runtime.h>

namespace dglhip {

namespace {

constexpr int kWave = 64;
constexpr int kMaxWaves = 16;
constexpr int64_t kLdsFloats = 32768;  // of the staged segment: 128 KiB
constexpr int64_t kMaxResident = DGLHIP_FPS_MAX_RESIDENT;
static_assert(kMaxResident == kMaxWaves * kWave * 8, "the largest resident kernel is 16 x 8");
static_assert(kMaxResident * 4 <= kLdsFloats, "its D <= 4 copy must fit");

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct FpsArgs {
  int64_t B, N, D, m, ldx;
  int rows;    // resident: the rows a workgroup holds at most (LDS and registers)
  int stride;  // resident: floats per staged row
  const int64_t* offsets;
  const float* x;
  const int64_t* start;
  int64_t* idx;
  float* dist;
  float* mind;  // general: the running minima, one per row of x
};

__device__ __forceinline__ int64_t clampi(int64_t v, int64_t lo, int64_t hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

__device__ __forceinline__ uint64_t key_of(float mind, uint32_t row) {
  const uint32_t hi = mind < 0.0f ? 0u : __float_as_uint(mind) + 1u;
  return (uint64_t(hi) << 32) | (~row);
}

// the running minimum after the pick at distance d; the pick itself is taken
__device__ __forceinline__ float relax(float mind, float d, bool picked) {
  const float v = d < mind ? d : mind;
  return picked ? -1.0f : v;
}

template <int CTRL>
__device__ __forceinline__ uint64_t dpp_max(uint64_t k) {
  const uint32_t lo = __builtin_amdgcn_update_dpp(0, static_cast<int>(k), CTRL, 0xF, 0xF, false);
  const uint32_t hi =
      __builtin_amdgcn_update_dpp(0, static_cast<int>(k >> 32), CTRL, 0xF, 0xF, false);
  const uint64_t o = (uint64_t(hi) << 32) | lo;
  return o > k ? o : k;
}

// every lane gets the largest key of its row of 16 lanes
__device__ __forceinline__ uint64_t row_max(uint64_t k) {
  k = dpp_max<0xB1>(k);   // quad_perm [1, 0, 3, 2]
  k = dpp_max<0x4E>(k);   // quad_perm [2, 3, 0, 1]
  k = dpp_max<0x141>(k);  // row_half_mirror
  return dpp_max<0x140>(k);  // row_mirror
}

__device__ __forceinline__ uint64_t read_lane(uint64_t k, int l) {
  const uint32_t lo = __builtin_amdgcn_readlane(static_cast<int>(k), l);
  const uint32_t hi = __builtin_amdgcn_readlane(static_cast<int>(k >> 32), l);
  return (uint64_t(hi) << 32) | lo;
}

// the largest key of the wave, uniform
__device__ __forceinline__ uint64_t wave_max(uint64_t k) {
  k = row_max(k);
  const uint64_t a = read_lane(k, 0), b = read_lane(k, 16);
  const uint64_t c = read_lane(k, 32), d = read_lane(k, 48);
  const uint64_t ab = a > b ? a : b, cd = c > d ? c : d;
  return ab > cd ? ab : cd;
}

// The largest key of the workgroup from the waves' keys: the one barrier of a
// pick. slots: 2 x kMaxWaves, unused entries 0.
template <int W>
__device__ __forceinline__ uint64_t group_max(uint64_t k, uint64_t* slots, int pick) {
  if constexpr (W > 1) {
    uint64_t* s = slots + (pick & 1) * kMaxWaves;
    if ((threadIdx.x & (kWave - 1)) == 0) s[threadIdx.x >> 6] = k;
    __syncthreads();
    k = read_lane(row_max(s[threadIdx.x & (kMaxWaves - 1)]), 0);
  }
  return k;
}

// what every kernel does first: the segment, its padding slots, the first pick
struct Segment {
  int64_t beg, len;
  int picks;
  uint32_t win;
  int64_t* idx;
  float* dist;
};

__device__ __forceinline__ Segment open_segment(const FpsArgs& a, int64_t s, int64_t max_len,
                                                int threads) {
  Segment g;
  g.beg = clampi(a.offsets[s], 0, a.N);
  g.len = clampi(a.offsets[s + 1], g.beg, a.N) - g.beg;
  if (g.len > max_len) g.len = max_len;
  g.picks = static_cast<int>(a.m < g.len ? a.m : g.len);
  g.idx = a.idx + s * a.m;
  g.dist = a.dist + s * a.m;
  for (int64_t j = g.picks + threadIdx.x; j < a.m; j += threads) {
    g.idx[j] = -1;
    g.dist[j] = 0.0f;
  }
  g.win = 0;
  if (a.start != nullptr && g.len > 0)
    g.win = static_cast<uint32_t>(clampi(a.start[s], 0, g.len - 1));
  return g;
}

template <int W, int RPL, bool kRegs>
__global__ __launch_bounds__(W * kWave) void segment_fps_kernel(FpsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float xs[];  // the segment: rows x stride
  __shared__ uint64_t slots[2 * kMaxWaves];
  constexpr int T = W * kWave;
  const int tid = threadIdx.x;
  const int64_t s = block_linear();
  if (s >= a.B) return;
  const Segment g = open_segment(a, s, a.rows, T);
  if (g.len == 0) return;  // the whole workgroup
  const int len = static_cast<int>(g.len), D = static_cast<int>(a.D), stride = a.stride;

  for (int e = tid; e < len * stride; e += T) {
    const int r = e / stride, c = e - r * stride;
    xs[e] = c < D ? a.x[(g.beg + r) * a.ldx + c] : 0.0f;
  }
  if (W > 1 && tid < 2 * kMaxWaves) slots[tid] = 0;
  __syncthreads();

  // lane tid owns rows tid, tid + T, ...
  float mind[RPL];
  f32x4 xr[RPL];
  const float* row[RPL];
#pragma unroll
  for (int r = 0; r < RPL; ++r) {
    const int j = tid + r * T;
    mind[r] = j < len ? __uint_as_float(0x7f800000u) : -1.0f;
    row[r] = xs + (j < len ? j : len - 1) * stride;  // past the end: a row to read, never picked
    if constexpr (kRegs) xr[r] = *reinterpret_cast<const f32x4*>(row[r]);
  }

  uint32_t win = g.win;
  float dwin = __uint_as_float(0x7f800000u);
  for (int i = 0;; ++i) {
    if (tid == 0) {
      g.idx[i] = g.beg + win;
      g.dist[i] = dwin;
    }
    if (i + 1 >= g.picks) break;
    float d[RPL];
#pragma unroll
    for (int r = 0; r < RPL; ++r) d[r] = 0.0f;
    if constexpr (kRegs) {
      const f32x4 p = *reinterpret_cast<const f32x4*>(xs + 4 * win);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int r = 0; r < RPL; ++r) {
          const float t = xr[r][c] - p[c];
          d[r] = fmaf(t, t, d[r]);
        }
      }
    } else {
      const float* prow = xs + win * stride;
      for (int c = 0; c < D; ++c) {
        const float p = prow[c];
#pragma unroll
        for (int r = 0; r < RPL; ++r) {
          const float t = row[r][c] - p;
          d[r] = fmaf(t, t, d[r]);
        }
      }
    }
    uint64_t best = 0;
#pragma unroll
    for (int r = 0; r < RPL; ++r) {
      const uint32_t j = tid + r * T;
      mind[r] = relax(mind[r], d[r], j == win);
      const uint64_t k = key_of(mind[r], j);
      best = k > best ? k : best;
    }
    best = group_max<W>(wave_max(best), slots, i);
    win = ~static_cast<uint32_t>(best);
    dwin = __uint_as_float(static_cast<uint32_t>(best >> 32) - 1u);
  }
}

constexpr int kGeneralWaves = kMaxWaves;

template <int V>
__global__ __launch_bounds__(kGeneralWaves * kWave) void segment_fps_general_kernel(FpsArgs a) {
  __shared__ uint64_t slots[2 * kMaxWaves];
  constexpr int T = kGeneralWaves * kWave;
  const int tid = threadIdx.x;
  const int64_t s = block_linear();
  if (s >= a.B) return;
  const Segment g = open_segment(a, s, a.N, T);
  if (g.len == 0) return;  // the whole workgroup
  const int64_t len = g.len, D = a.D;
  float* mind = a.mind + g.beg;
  for (int64_t j = tid; j < len; j += T) mind[j] = __uint_as_float(0x7f800000u);
  if (tid < 2 * kMaxWaves) slots[tid] = 0;
  __syncthreads();

  uint32_t win = g.win;
  float dwin = __uint_as_float(0x7f800000u);
  for (int i = 0;; ++i) {
    if (tid == 0) {
      g.idx[i] = g.beg + win;
      g.dist[i] = dwin;
    }
    if (i + 1 >= g.picks) break;
    const float* prow = a.x + (g.beg + win) * a.ldx;
    uint64_t best = 0;
    for (int64_t j = tid; j < len; j += T) {
      const float* row = a.x + (g.beg + j) * a.ldx;
      float d = 0.0f;
      if constexpr (V == 4) {
        for (int64_t c = 0; c < D; c += 4) {
          const f32x4 q = *reinterpret_cast<const f32x4*>(row + c);
          const f32x4 p = *reinterpret_cast<const f32x4*>(prow + c);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float t = q[u] - p[u];
            d = fmaf(t, t, d);
          }
        }
      } else {
        for (int64_t c = 0; c < D; ++c) {
          const float t = row[c] - prow[c];
          d = fmaf(t, t, d);
        }
      }
      const float v = relax(mind[j], d, j == win);
      mind[j] = v;
      const uint64_t k = key_of(v, static_cast<uint32_t>(j));
      best = k > best ? k : best;
    }
    best = group_max<kGeneralWaves>(wave_max(best), slots, i);
    win = ~static_cast<uint32_t>(best);
    dwin = __uint_as_float(static_cast<uint32_t>(best >> 32) - 1u);
  }
}

int64_t stride_of(int64_t D) { return D <= 4 ? 4 : (D | 1); }

// the resident kernels serve a launch whose longest segment is known and fits
bool resident(int64_t D, int64_t max_rows) {
  return max_rows >= 0 && max_rows <= kMaxResident && max_rows * stride_of(D) <= kLdsFloats;
}

template <int W, int RPL, bool kRegs>
void launch_resident(const FpsArgs& a, hipStream_t stream) {
  const size_t lds = static_cast<size_t>(a.rows) * a.stride * sizeof(float);
  const auto kernel = segment_fps_kernel<W, RPL, kRegs>;
  if (lds > 48 * 1024)
    DGLHIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                     static_cast<int>(lds)) == hipSuccess,
                 "segment fps: " << lds << " bytes of LDS refused");
  hipLaunchKernelGGL(kernel, grid_1d(a.B), dim3(W * kWave), lds, stream, a);
}

template <bool kRegs>
void launch_by_rows(const FpsArgs& a, hipStream_t stream) {
  if (a.rows <= 64) launch_resident<1, 1, kRegs>(a, stream);
  else if (a.rows <= 256) launch_resident<1, 4, kRegs>(a, stream);
  else if (a.rows <= 1024) launch_resident<4, 4, kRegs>(a, stream);
  else if (a.rows <= 4096) launch_resident<16, 4, kRegs>(a, stream);
  else launch_resident<16, 8, kRegs>(a, stream);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

}  // namespace dglhip

using namespace dglhip;

extern "C" {

int64_t dglhip_segment_fps_workspace_bytes(int64_t num_segments, int64_t num_rows, int64_t dim,
                                           int64_t m, int64_t max_segment_rows) {
  if (num_segments <= 0 || num_rows <= 0 || dim < 1 || m < 1) return 0;
  if (max_segment_rows > num_rows) max_segment_rows = num_rows;
  return resident(dim, max_segment_rows) ? 0 : num_rows * 4;
}

int dglhip_segment_fps_device(int64_t num_segments, int64_t num_rows, int64_t dim, int64_t m,
                              const int64_t* offsets, const float* x, int64_t ldx,
                              const int64_t* start, int64_t* idx, float* dist,
                              int64_t max_segment_rows, void* workspace, void* stream_) {
  API_BEGIN();
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  DGLHIP_CHECK(num_segments >= 0 && num_rows >= 0, "negative size");
  DGLHIP_CHECK(m >= 1, "m = " << m << " picks");
  DGLHIP_CHECK(dim >= 1 && dim <= DGLHIP_FPS_MAX_DIM,
               "D = " << dim << " outside [1, DGLHIP_FPS_MAX_DIM = " << DGLHIP_FPS_MAX_DIM << "]");
  DGLHIP_CHECK(num_rows < (int64_t(1) << 31), "num_rows must be below 2^31");
  if (num_segments == 0) return 0;
  DGLHIP_CHECK(offsets && idx && dist && (num_rows == 0 || x), "null pointer argument");
  DGLHIP_CHECK(ldx >= dim, "row stride below the row width");
  if (max_segment_rows > num_rows) max_segment_rows = num_rows;
  FpsArgs a;
  a.B = num_segments; a.N = num_rows; a.D = dim; a.m = m; a.ldx = ldx;
  a.offsets = offsets; a.x = x; a.start = start; a.idx = idx; a.dist = dist;
  a.mind = static_cast<float*>(workspace);
  a.rows = 0;
  a.stride = static_cast<int>(stride_of(dim));
  if (resident(dim, max_segment_rows)) {
    a.rows = static_cast<int>(std::max<int64_t>(max_segment_rows, 1));
    if (dim <= 4) launch_by_rows<true>(a, stream);
    else launch_by_rows<false>(a, stream);
  } else {
    DGLHIP_CHECK(workspace || num_rows == 0, "segments of unknown or long size need the workspace");
    const dim3 grid = grid_1d(a.B), block(kGeneralWaves * kWave);
    if (dim % 4 == 0 && ldx % 4 == 0 && aligned16(x))
      hipLaunchKernelGGL((segment_fps_general_kernel<4>), grid, block, 0, stream, a);
    else
      hipLaunchKernelGGL((segment_fps_general_kernel<1>), grid, block, 0, stream, a);
  }
  DGLHIP_CHECK(hipGetLastError() == hipSuccess, "segment fps launch failed");
  API_END();
}

}  // extern "C"
