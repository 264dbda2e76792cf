// Segment top-k: the k first rows of every segment in sorted order, the
// readout behind topk_nodes / topk_edges and SortPooling, and its backward.
//
// sortby < 0: every column of segment s is ranked on its own, values[s, j, f]
// is the j-th element of column f and indices[s, j, f] its row within the
// segment. sortby = c: whole rows are ranked by column c, values[s, j, :] is
// the j-th row and indices[s, j] its row within the segment. Slots past the
// end of a short segment hold +0.0f and -1.
//
// Key. A float becomes a 32-bit key whose unsigned order is the float order
// (non-negatives get the sign bit set, negatives are complemented, -0.0 is
// keyed as +0.0, every NaN is 0xffffffff), complemented when descending; the
// packed word is key << 32 | row within the segment. The smaller word comes
// first: one unsigned compare is the whole total order of a stable sort (NaN
// first when descending and last when ascending, equal keys by row). The order
// is strict, so the result does not depend on how the rows are cut or merged.
// Values are never rebuilt from keys: the output is read from x at the row the
// word names, so signs of zero and NaN payloads pass through.
//
// Mapping. A workgroup of 256 lanes owns kSlots packed words of LDS (64 KiB).
// An item is one chunk of at most DGLHIP_TOPK_CHUNK rows of a segment by a
// tile of T columns. The lanes read the rows with consecutive lanes on
// consecutive columns (16 bytes per lane where F % 4 == 0 and the rows are
// aligned) and store the words transposed, column t of the tile as the
// sub-array [t * stride, t * stride + P), P the power of two >= the rows:
// stride is P + 1 below a full chunk, so the T lanes of a row spread over the
// banks. All sub-arrays are sorted together by one bitonic network over the
// workgroup, a compare-exchange per lane and step. The output is written with
// lanes on consecutive columns again. The launch picks T and, when the caller
// knows that every segment is short, packs S segments into one workgroup
// (S * T * stride <= kSlots), so a batch of 30-row graphs sorts 3 segments x
// 64 columns per workgroup. With sortby = c the tile is the one key column,
// S segments per workgroup, and the same workgroup then copies the k selected
// rows whole, coalesced: no argsort of the rows goes through memory.
//
// Long segments, from the sizes alone (no host sync): item s < B is the first
// chunk of segment s; item B + g belongs to the block of rows [g C, (g + 1) C)
// and is the later chunk that starts in it (at most one, of the segment that
// contains row g C: found by a binary search of the offsets). A later chunk
// writes its min(k, rows) best words to slot g of the workspace, the first
// chunk of a long segment writes its k best words into the index output
// (int64 like the words) in place. A second launch, one workgroup per (long
// segment, column), sorts the running best k with as many chunk lists as fit
// in LDS per round and writes the final values and indices. A caller that
// knows the longest segment passes it; the block items and the second launch
// are skipped when it is <= C.
//
// Backward: dx[beg[s] + indices[s, j, f], f] = dy[s, j, f], zero elsewhere. A
// workgroup owns 256 rows x 64 columns of dx: it scatters the ranks j of the
// selected elements of its block into an LDS table (int16, -1 elsewhere), then
// writes its block of dx once, coalesced, reading dy[s, rank, f] where the
// table names one. No atomics; every dx element is written exactly once.
#include "../../include/dgl_hip.h"
#include "common.h"
#include "launch.h"

#include <hip/hip_runtime.h>

namespace dglhip {

namespace {

constexpr int kThreads = 256;
constexpr int64_t kChunk = DGLHIP_TOPK_CHUNK;
constexpr int kSlots = 8192;  // packed words of LDS per workgroup: 64 KiB
constexpr int kMaxPack = 8;   // segments per workgroup at most
constexpr int kMaxTile = 64;  // columns per tile at most
constexpr uint64_t kAbsent = ~uint64_t(0);  // sorts after every word of a row
constexpr int kBwdRows = 256, kBwdCols = 64;
static_assert(kSlots / kChunk >= 4 && kSlots >= 2 * kChunk, "a chunk by 4 columns must fit");
static_assert(kBwdRows == kThreads, "one lane per row finds the row's segment");
static_assert(kChunk <= 32768, "the backward keeps ranks in int16");

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

__device__ __forceinline__ uint64_t pack_key(float v, uint32_t pos, bool desc) {
  uint32_t b = __float_as_uint(v);
  uint32_t key = 0xffffffffu;
  if (v == v) {
    if (b == 0x80000000u) b = 0u;
    key = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  }
  if (desc) key = ~key;
  return (uint64_t(key) << 32) | pos;
}

__device__ __forceinline__ int ceil_log2(int64_t n) {
  int l = 0;
  while ((int64_t(1) << l) < n) ++l;
  return l;
}

// Ascending bitonic sort of nsub sub-arrays of 2^logp words, sub-array q at
// a + q * stride, by the whole workgroup. The words must be visible (a
// barrier after the stores) on entry and are on return.
__device__ void sort_lds(uint64_t* a, int nsub, int stride, int logp) {
  const int half = 1 << (logp - 1), total = nsub << (logp - 1), P = 1 << logp;
  for (int kk = 2; kk <= P; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int idx = threadIdx.x; idx < total; idx += kThreads) {
        const int q = idx >> (logp - 1), h = idx & (half - 1);
        const int i = ((h & ~(j - 1)) << 1) | (h & (j - 1));
        uint64_t* p = a + q * stride;
        const uint64_t lo = p[i], hi = p[i | j];
        const bool up = (i & kk) == 0;
        if ((lo > hi) == up) {
          p[i] = hi;
          p[i | j] = lo;
        }
      }
      __syncthreads();
    }
  }
}

struct TopkArgs {
  int64_t B, N, F, k, G;  // G block items (0: no segment is longer than a chunk)
  int64_t ldx;
  int64_t sortby;  // the key column, -1: every column
  int desc;
  int vec;     // 16-byte row copies (sortby >= 0)
  int logp;    // log2 of the sort size of a packed launch (S > 1)
  int logt;    // log2 of the columns per tile T
  int S;       // segments per workgroup (1 when G > 0)
  int64_t tiles;
  const int64_t* offsets;
  const float* x;
  float* values;
  int64_t* indices;
  uint64_t* ws;  // G x (F or 1) x k words
};

enum { kOutFinal = 0, kOutFirst = 1, kOutSlot = 2, kOutNone = 3 };

// what a workgroup sorts for one item: rows [r0, r0 + n) of segment s (which
// starts at row beg), and where the result goes
struct Item {
  int64_t s, beg, r0, slot;
  int n, out;
};

__device__ __forceinline__ Item item_of(const TopkArgs& a, int64_t item) {
  Item it = {0, 0, 0, 0, 0, kOutNone};
  if (item < a.B) {
    it.s = item;
    it.beg = clampi(a.offsets[item], 0, a.N);
    const int64_t end = clampi(a.offsets[item + 1], it.beg, a.N);
    const int64_t len = end - it.beg;
    it.r0 = it.beg;
    it.n = static_cast<int>(len > kChunk ? kChunk : len);
    it.out = (len > kChunk && a.G > 0) ? kOutFirst : kOutFinal;
  } else if (item < a.B + a.G) {
    const int64_t g = item - a.B, row0 = g * kChunk;
    const int64_t s = segment_of(a.offsets, a.B, row0);
    if (s >= a.B) return it;
    const int64_t beg = clampi(a.offsets[s], 0, a.N);
    const int64_t end = clampi(a.offsets[s + 1], beg, a.N);
    if (row0 < beg) return it;
    const int64_t q = (row0 - beg + kChunk - 1) / kChunk;
    const int64_t p = beg + q * kChunk;
    if (q < 1 || p >= end || p >= row0 + kChunk) return it;
    it.s = s; it.beg = beg; it.r0 = p; it.slot = g;
    it.n = static_cast<int>(end - p > kChunk ? kChunk : end - p);
    it.out = kOutSlot;
  }
  // a caller that understated the longest segment gets its first rows ranked
  if (it.n > (1 << a.logp)) it.n = 1 << a.logp;
  return it;
}

template <int V>
__global__ __launch_bounds__(kThreads) void segment_topk_kernel(TopkArgs a) {
  __shared__ uint64_t keys[kSlots];
  const bool rows = a.sortby >= 0;
  const int tid = threadIdx.x;
  const int64_t wg = block_linear();
  const int64_t group = wg / a.tiles, tile = wg - group * a.tiles;
  // one item: its own sort size; a packed launch (no block items): the launch's
  int logp = a.logp;
  if (a.S == 1) {
    const Item it = item_of(a, group);
    if (it.out == kOutNone) return;  // the whole workgroup
    logp = ceil_log2(it.n);
    if (logp < 1) logp = 1;
  }
  const int P = 1 << logp;
  const int stride = P < kChunk ? P + 1 : P;
  const int T = 1 << a.logt;
  const bool desc = a.desc != 0;
  const int64_t c0 = rows ? a.sortby : tile * T;

  // rows -> words, transposed: lanes on consecutive columns of a row
  for (int sl = 0; sl < a.S; ++sl) {
    const Item it = item_of(a, group * a.S + sl);
    constexpr int LV = V == 4 ? 2 : 0;
    const int logtv = a.logt - LV;  // lanes per row of the tile
    uint64_t* sub = keys + sl * T * stride;
    for (int e = tid; e < P << logtv; e += kThreads) {
      const int r = e >> logtv, t = (e & ((1 << logtv) - 1)) << LV;
      const bool live = r < it.n && (rows || c0 + t < a.F);
      float v[V];
#pragma unroll
      for (int u = 0; u < V; ++u) v[u] = 0.0f;
      if (live) {
        const float* p = a.x + (it.r0 + r) * a.ldx + c0 + t;
        if constexpr (V == 4) {
          const f32x4 q = *reinterpret_cast<const f32x4*>(p);
          v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
        } else {
          v[0] = *p;
        }
      }
      const uint32_t pos = static_cast<uint32_t>(it.r0 - it.beg) + r;
#pragma unroll
      for (int u = 0; u < V; ++u)
        sub[(t + u) * stride + r] = live ? pack_key(v[u], pos, desc) : kAbsent;
    }
  }
  __syncthreads();
  sort_lds(keys, a.S * T, stride, logp);

  for (int sl = 0; sl < a.S; ++sl) {
    const Item it = item_of(a, group * a.S + sl);
    if (it.out == kOutNone) continue;
    const int64_t s = it.s, beg = it.beg;
    const int n = it.n;
    const uint64_t* sub = keys + sl * T * stride;
    if (it.out == kOutFirst) {  // a long segment's first chunk: n == kChunk >= k
      const int64_t Fi = rows ? 1 : a.F;
      for (int64_t e = tid; e < a.k << a.logt; e += kThreads) {
        const int64_t j = e >> a.logt;
        const int t = static_cast<int>(e & (T - 1));
        if (!rows && c0 + t >= a.F) continue;
        a.indices[(s * a.k + j) * Fi + (rows ? 0 : c0 + t)] =
            static_cast<int64_t>(sub[t * stride + j]);
      }
    } else if (it.out == kOutSlot) {  // lanes on consecutive words of a list
      const int64_t cnt = a.k < n ? a.k : n, Fe = rows ? 1 : a.F;
      for (int64_t e = tid; e < cnt << a.logt; e += kThreads) {
        const int t = static_cast<int>(e / cnt);
        const int64_t j = e - t * cnt;
        if (!rows && c0 + t >= a.F) continue;
        a.ws[(it.slot * Fe + (rows ? 0 : c0 + t)) * a.k + j] = sub[t * stride + j];
      }
    } else if (!rows) {
      for (int64_t e = tid; e < a.k << a.logt; e += kThreads) {
        const int64_t j = e >> a.logt;
        const int t = static_cast<int>(e & (T - 1));
        const int64_t col = c0 + t;
        if (col >= a.F) continue;
        float val = 0.0f;
        int64_t idx = -1;
        if (j < n) {
          idx = static_cast<uint32_t>(sub[t * stride + j]);
          val = a.x[(beg + idx) * a.ldx + col];
        }
        const int64_t o = (s * a.k + j) * a.F + col;
        a.values[o] = val;
        a.indices[o] = idx;
      }
    } else if (a.vec) {  // the selected rows, 16 bytes per lane
      const int64_t F4 = a.F >> 2;
      for (int64_t e = tid; e < a.k * F4; e += kThreads) {
        const int64_t j = e / F4, c = (e - j * F4) << 2;
        f32x4 q = {0.0f, 0.0f, 0.0f, 0.0f};
        int64_t idx = -1;
        if (j < n) {
          idx = static_cast<uint32_t>(sub[j]);
          q = *reinterpret_cast<const f32x4*>(a.x + (beg + idx) * a.ldx + c);
        }
        *reinterpret_cast<f32x4*>(a.values + (s * a.k + j) * a.F + c) = q;
        if (c == 0) a.indices[s * a.k + j] = idx;
      }
    } else {
      for (int64_t e = tid; e < a.k * a.F; e += kThreads) {
        const int64_t j = e / a.F, c = e - j * a.F;
        float val = 0.0f;
        int64_t idx = -1;
        if (j < n) {
          idx = static_cast<uint32_t>(sub[j]);
          val = a.x[(beg + idx) * a.ldx + c];
        }
        a.values[(s * a.k + j) * a.F + c] = val;
        if (c == 0) a.indices[s * a.k + j] = idx;
      }
    }
  }
}

// The second launch: workgroup (s, f) of a segment of more than one chunk
// (f = 0 with sortby >= 0) keeps the best k words in keys[0, k), appends as
// many chunk lists of k words as fit, sorts, and repeats until the lists are
// used up; then it writes the final values and indices of its column (rows).
__global__ __launch_bounds__(kThreads) void segment_topk_merge_kernel(TopkArgs a) {
  __shared__ uint64_t keys[kSlots];
  const bool rows = a.sortby >= 0;
  const int tid = threadIdx.x;
  const int64_t Fe = rows ? 1 : a.F;
  const int64_t wg = block_linear();
  if (wg >= a.B * Fe) return;
  const int64_t s = wg / Fe, f = wg - s * Fe;
  const int64_t beg = clampi(a.offsets[s], 0, a.N);
  const int64_t end = clampi(a.offsets[s + 1], beg, a.N);
  const int64_t len = end - beg;
  if (len <= kChunk) return;
  const int64_t g1 = (beg + kChunk) / kChunk;  // the slot of chunk q is g1 + q - 1
  const int64_t nk = (len + kChunk - 1) / kChunk;
  const int k = static_cast<int>(a.k);
  for (int j = tid; j < k; j += kThreads)
    keys[j] = static_cast<uint64_t>(a.indices[(s * a.k + j) * Fe + f]);
  const int64_t lists = (kSlots - k) / k;  // chunk lists per round, >= 1
  for (int64_t q0 = 1; q0 < nk; q0 += lists) {
    const int64_t m = nk - q0 < lists ? nk - q0 : lists;
    const int used = k + static_cast<int>(m) * k;
    const int logp = ceil_log2(used);
    for (int e = k + tid; e < (1 << logp); e += kThreads) {
      uint64_t w = kAbsent;
      if (e < used) {
        const int64_t q = q0 + (e - k) / k;
        const int j = (e - k) % k;
        const int64_t crow = beg + q * kChunk;
        const int64_t cnt = end - crow < a.k ? end - crow : a.k;
        if (j < cnt) w = a.ws[((g1 + q - 1) * Fe + f) * a.k + j];
      }
      keys[e] = w;
    }
    __syncthreads();
    sort_lds(keys, 1, 0, logp);
  }
  // a long segment has more than k rows, so all k slots are rows; a word that
  // names no row of the segment (offsets that changed under the launches) is
  // written as padding, never followed
  if (!rows) {
    for (int j = tid; j < k; j += kThreads) {
      int64_t idx = static_cast<uint32_t>(keys[j]);
      float val = 0.0f;
      if (idx < len) val = a.x[(beg + idx) * a.ldx + f];
      else idx = -1;
      const int64_t o = (s * a.k + j) * a.F + f;
      a.values[o] = val;
      a.indices[o] = idx;
    }
  } else {
    for (int64_t e = tid; e < a.k * a.F; e += kThreads) {
      const int64_t j = e / a.F, c = e - j * a.F;
      int64_t idx = static_cast<uint32_t>(keys[j]);
      float val = 0.0f;
      if (idx < len) val = a.x[(beg + idx) * a.ldx + c];
      else idx = -1;
      a.values[(s * a.k + j) * a.F + c] = val;
      if (c == 0) a.indices[s * a.k + j] = idx;
    }
  }
}

struct TopkBwdArgs {
  int64_t B, N, F, k;
  int rows;  // sortby >= 0: indices is (B, k) and whole rows move
  int64_t tiles;
  const int64_t* offsets;
  const float* dy;
  const int64_t* indices;
  float* dx;
};

__global__ __launch_bounds__(kThreads) void segment_topk_bwd_kernel(TopkBwdArgs a) {
  __shared__ int16_t rank[kBwdRows * kBwdCols];
  __shared__ int64_t s_seg[kBwdRows];
  const int tid = threadIdx.x;
  const int64_t wg = block_linear();
  const int64_t blk = wg / a.tiles, tile = wg - blk * a.tiles;
  const int64_t R0 = blk * kBwdRows, c0 = tile * kBwdCols;
  if (R0 >= a.N) return;  // the whole workgroup
  const int nrows = static_cast<int>(a.N - R0 < kBwdRows ? a.N - R0 : kBwdRows);
  const int logt = a.rows ? 0 : 6;  // table columns: one rank per row, or per element
  for (int e = tid; e < kBwdRows << logt; e += kThreads) rank[e] = -1;
  {
    int64_t s = a.B - 1;
    if (tid < nrows) {
      s = segment_of(a.offsets, a.B, R0 + tid);
      if (s >= a.B) s = a.B - 1;
    }
    s_seg[tid] = s;
  }
  __syncthreads();
  const int64_t s_first = s_seg[0], s_last = s_seg[nrows - 1];
  for (int64_t s = s_first; s <= s_last; ++s) {
    const int64_t beg = clampi(a.offsets[s], 0, a.N);
    const int64_t end = clampi(a.offsets[s + 1], beg, a.N);
    const int64_t cnt = end - beg < a.k ? end - beg : a.k;  // later slots are padding
    for (int64_t e = tid; e < cnt << logt; e += kThreads) {
      const int64_t j = e >> logt;
      const int t = static_cast<int>(e & ((1 << logt) - 1));
      if (!a.rows && c0 + t >= a.F) continue;
      const int64_t idx = a.rows ? a.indices[s * a.k + j] : a.indices[(s * a.k + j) * a.F + c0 + t];
      if (idx < 0) continue;
      const int64_t row = beg + idx;
      if (row >= R0 && row < R0 + nrows && row < end)
        rank[((row - R0) << logt) + t] = static_cast<int16_t>(j);
    }
  }
  __syncthreads();
  for (int e = tid; e < nrows * kBwdCols; e += kThreads) {
    const int r = e >> 6, t = e & 63;
    const int64_t col = c0 + t;
    if (col >= a.F) continue;
    const int j = rank[a.rows ? r : (r << 6) + t];
    float g = 0.0f;
    if (j >= 0) g = a.dy[(s_seg[r] * a.k + j) * a.F + col];
    a.dx[(R0 + r) * a.F + col] = g;
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int64_t block_items(int64_t N) { return (N + kChunk - 1) / kChunk; }

void check_sizes(int64_t B, int64_t N, int64_t F, int64_t k, int64_t sortby) {
  DGLHIP_CHECK(B >= 0 && N >= 0 && F >= 0, "negative size");
  DGLHIP_CHECK(k >= 1 && k <= kChunk, "k = " << k << " outside [1, DGLHIP_TOPK_CHUNK = "
                                             << kChunk << "]");
  DGLHIP_CHECK(sortby >= -1 && (sortby < F || F == 0), "sortby " << sortby << " is no column");
  DGLHIP_CHECK(N < (int64_t(1) << 32) - 1, "rows within a segment are kept in 32 bits");
}

}  // namespace

}  // namespace dglhip

using namespace dglhip;

extern "C" {

int64_t dglhip_segment_topk_workspace_bytes(int64_t num_segments, int64_t num_rows,
                                            int64_t feat_len, int64_t k, int descending,
                                            int64_t sortby) {
  (void)descending;
  if (num_rows <= kChunk || num_segments <= 0 || feat_len <= 0 || k < 1 || k > kChunk) return 0;
  return block_items(num_rows) * (sortby >= 0 ? 1 : feat_len) * k * 8;
}

int dglhip_segment_topk_device(int64_t num_segments, int64_t num_rows, int64_t feat_len,
                               int64_t k, int descending, int64_t sortby,
                               const int64_t* offsets, const float* x, int64_t ldx,
                               float* values, int64_t* indices, int64_t max_segment_rows,
                               void* workspace, void* stream_) {
  API_BEGIN();
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  check_sizes(num_segments, num_rows, feat_len, k, sortby);
  if (num_segments == 0 || feat_len == 0) return 0;
  DGLHIP_CHECK(offsets && values && indices && (num_rows == 0 || x), "null pointer argument");
  DGLHIP_CHECK(ldx >= feat_len, "row stride below the row width");
  const bool rows = sortby >= 0;
  const bool chunks = num_rows > kChunk && (max_segment_rows < 0 || max_segment_rows > kChunk);
  DGLHIP_CHECK(!chunks || workspace, "segments longer than a chunk need the workspace");
  TopkArgs a;
  a.B = num_segments; a.N = num_rows; a.F = feat_len; a.k = k;
  a.G = chunks ? block_items(num_rows) : 0;
  a.ldx = ldx; a.sortby = sortby; a.desc = descending ? 1 : 0;
  a.offsets = offsets; a.x = x; a.values = values; a.indices = indices;
  a.ws = static_cast<uint64_t*>(workspace);
  // the longest item of the launch decides how many columns and segments a
  // workgroup's LDS holds
  int64_t longest = chunks ? kChunk : (max_segment_rows >= 0 ? max_segment_rows : num_rows);
  if (longest > num_rows) longest = num_rows;
  if (longest > kChunk) longest = kChunk;
  a.logp = 1;
  while ((int64_t(1) << a.logp) < longest) ++a.logp;
  const int64_t P = int64_t(1) << a.logp;
  const int64_t cap = P < kChunk ? kSlots / (P + 1) : kSlots / P;  // sub-arrays per workgroup
  const int64_t Fe = rows ? 1 : feat_len;
  a.logt = 0;
  while ((1 << a.logt) < kMaxTile && (int64_t(1) << a.logt) < Fe && (int64_t(2) << a.logt) <= cap)
    ++a.logt;
  const int64_t T = int64_t(1) << a.logt;
  a.S = 1;
  if (!chunks) a.S = static_cast<int>(std::min<int64_t>(kMaxPack, std::max<int64_t>(1, cap / T)));
  a.tiles = (Fe + T - 1) / T;
  const bool vec4 = feat_len % 4 == 0 && ldx % 4 == 0 && aligned16(x);
  a.vec = vec4 && aligned16(values) ? 1 : 0;
  const int64_t groups = (a.B + a.G + a.S - 1) / a.S;
  const dim3 grid = grid_1d(groups * a.tiles);
  if (!rows && vec4)
    hipLaunchKernelGGL((segment_topk_kernel<4>), grid, dim3(kThreads), 0, stream, a);
  else
    hipLaunchKernelGGL((segment_topk_kernel<1>), grid, dim3(kThreads), 0, stream, a);
  DGLHIP_CHECK(hipGetLastError() == hipSuccess, "segment top-k launch failed");
  if (chunks) {
    hipLaunchKernelGGL(segment_topk_merge_kernel, grid_1d(a.B * Fe), dim3(kThreads), 0, stream, a);
    DGLHIP_CHECK(hipGetLastError() == hipSuccess, "segment top-k merge launch failed");
  }
  API_END();
}

int dglhip_segment_topk_bwd_device(int64_t num_segments, int64_t num_rows, int64_t feat_len,
                                   int64_t k, int descending, int64_t sortby,
                                   const int64_t* offsets, const float* dy,
                                   const int64_t* indices, float* dx, void* stream_) {
  API_BEGIN();
  (void)descending;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  check_sizes(num_segments, num_rows, feat_len, k, sortby);
  if (num_rows == 0 || feat_len == 0) return 0;
  DGLHIP_CHECK(num_segments >= 1, "rows without a segment");
  DGLHIP_CHECK(offsets && dy && indices && dx, "null pointer argument");
  TopkBwdArgs a;
  a.B = num_segments; a.N = num_rows; a.F = feat_len; a.k = k;
  a.rows = sortby >= 0 ? 1 : 0;
  a.tiles = (feat_len + kBwdCols - 1) / kBwdCols;
  a.offsets = offsets; a.dy = dy; a.indices = indices; a.dx = dx;
  const int64_t blocks = (num_rows + kBwdRows - 1) / kBwdRows;
  hipLaunchKernelGGL(segment_topk_bwd_kernel, grid_1d(blocks * a.tiles), dim3(kThreads), 0,
                     stream, a);
  DGLHIP_CHECK(hipGetLastError() == hipSuccess, "segment top-k backward launch failed");
  API_END();
}

}  // extern "C"
