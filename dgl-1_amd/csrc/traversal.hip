// Level-synchronous BFS and topological (Kahn) frontiers of a graph whose CSR
// is on the device: the device route of dgl.bfs_nodes_generator,
// bfs_edges_generator and topological_nodes_generator.
//
// The answer is that of the host queue loops of graph_traversal.cc, element for
// element and in the same order, on every run. The host loop looks at the
// slots of the frontier's rows one after the other; slot number c of that
// concatenation is *candidate* c. BFS gives an unvisited node to the first
// candidate that reaches it (the minimum c); Kahn releases a node at the
// candidate that does its last decrement (the maximum c of the level). So the
// winning candidates, in order of c, are the host's next queue segment.
//
// One level (dglhip_traversal_level_device) is a fixed sequence of launches
// over the frontier front[0..f), whose candidate total C the caller read from
// the previous status:
//   1. degrees: deg[i] of front[i] and its ceil(deg / K) items of at most K =
//      DGLHIP_TRAVERSAL_CHUNK slots; BFS marks front[i] visited here, which
//      is after the previous level's last read of `visited` and before this
//      level's first. Both are scanned (rocPRIM): cand_ptr[i] is the candidate
//      index of row i's first slot, item_ptr[i] its first item. Every item
//      finds its row by the shared item-row search (compact.h).
//   2. claim, one wave per item, lane k reads slot base + k. BFS: an unvisited
//      target v gets atomicMin(claim[v], c). Topological: remain[v] is
//      decremented and atomicMax(claim[v], key_base + c), where key_base is
//      one plus the candidates of all earlier levels, so keys grow from level
//      to level and `claim` is never reset.
//   3. count, the same walk: candidate c wins when (BFS) v is unvisited and
//      claim[v] == c, or (topological) remain[v] == 0 and claim[v] ==
//      key_base + c. Winners per item are counted and scanned.
//   4. fill, the same walk: a winner's position is its item's scanned base,
//      plus the winners of the item's earlier strides, plus the popcount of the
//      wave ballot below its lane. next[pos] = v, and for BFS edges
//      next_edge[pos] = eid[slot]. The winners' degrees are summed into the
//      status: the candidate total of the next level.
// The atomics decide which candidate wins, never a position; every output
// element is written once. Visibility between the stages is the kernel
// boundary: no kernel waits on another workgroup, and the level loop is the
// caller's, with one host read of the status per level.
//
// Mapping: one wave per item, four items per 256-lane workgroup; index loads
// are whole 256-byte runs and the probes of visited / remain / claim are the
// random part, four strides of them in flight per wave.
#include "../../include/dgl_hip.h"
#include "compact.h"

namespace dglhip {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int64_t kChunk = DGLHIP_TRAVERSAL_CHUNK;
constexpr int kUnroll = 4;  // strides whose probes are in flight together
constexpr int kBfs = DGLHIP_TRAVERSE_BFS;
constexpr int kTopo = DGLHIP_TRAVERSE_TOPOLOGICAL;

using u64 = unsigned long long;

static_assert(kChunk % (64 * kUnroll) == 0, "a chunk is a whole number of unrolled strides");

// Items of a frontier of f rows holding C slots: sum of ceil(deg / K) <= f + C / K.
int64_t item_bound(int64_t f, int64_t C) { return f + C / kChunk + 1; }

// The workspace of one level (all sections 256-byte aligned).
struct Layout {
  int64_t bound;
  int64_t deg, nit, cand_ptr, item_ptr, item_row, item_cnt, item_base, scan, scan_len, total;
  Layout(int64_t f, int64_t C) {
    bound = item_bound(f, C);
    Carve c;
    deg = c.take(f * 8);
    nit = c.take(f * 8);
    cand_ptr = c.take((f + 1) * 8);
    item_ptr = c.take((f + 1) * 8);
    item_row = c.take(bound * 4);
    item_cnt = c.take(bound * 8);
    item_base = c.take((bound + 1) * 8);
    const size_t s0 = scan_bytes_i64(f), s1 = scan_bytes_i64(bound);
    scan_len = round256(int64_t(s0 > s1 ? s0 : s1));
    scan = c.take(scan_len);
    total = c.off;
  }
};

struct Args {
  int64_t N, nnz, f, bound, key_base, cap;
  const int64_t* indptr;
  const int32_t* indices;
  const int64_t* eid;
  const int64_t* front;
  u64* claim;
  uint8_t* visited;  // BFS
  int64_t* remain;   // topological
  int64_t* deg;
  int64_t* nit;
  int64_t* cand_ptr;
  int64_t* item_ptr;
  int32_t* item_row;
  int64_t* item_cnt;
  int64_t* item_base;
  int64_t* next;
  int64_t* next_edge;
  int64_t* status;
};

// Source validation and the first candidate total: status = {n, sum of the
// in-range sources' degrees, ids outside [0, N)}.
__global__ __launch_bounds__(kThreads) void trv_source_kernel(int64_t N, int64_t nnz, int64_t n,
                                                              const int64_t* indptr,
                                                              const int64_t* source,
                                                              int64_t* status) {
  const int64_t i = block_linear() * kThreads + threadIdx.x;
  bool bad = false;
  int64_t deg = 0;
  if (i < n) {
    const int64_t v = source[i];
    if (v < 0 || v >= N) {
      bad = true;
    } else {
      int64_t b, e;
      row_range(indptr, nnz, v, &b, &e);
      deg = e - b;
    }
  }
  wave_count(bad, status + 2);
  wave_add(deg, status + 1);
  if (i == 0) status[0] = n;
}

// The status and the leading zero of each scanned array, in one launch.
__global__ void trv_reset_kernel(Args a) {
  if (threadIdx.x < 4) a.status[threadIdx.x] = 0;
  if (threadIdx.x == 4) a.cand_ptr[0] = 0;
  if (threadIdx.x == 5) a.item_ptr[0] = 0;
  if (threadIdx.x == 6) a.item_base[0] = 0;
}

__global__ __launch_bounds__(kThreads) void trv_degree_kernel(Args a) {
  const int64_t i = block_linear() * kThreads + threadIdx.x;
  bool bad = false;
  if (i < a.f) {
    const int64_t v = a.front[i];
    int64_t deg = 0;
    if (v < 0 || v >= a.N) {
      bad = true;  // counted, never used as an index
    } else {
      if (a.visited) a.visited[v] = 1;
      int64_t b, e;
      row_range(a.indptr, a.nnz, v, &b, &e);
      deg = e - b;
    }
    a.deg[i] = deg;
    a.nit[i] = (deg + kChunk - 1) / kChunk;
  }
  wave_count(bad, a.status + 2);
}

// The slots [beg, end) of item j and the candidate index of slot beg; false
// for an item past the end.
__device__ __forceinline__ bool item_range(const Args& a, int64_t j, int64_t* beg, int64_t* end,
                                           int64_t* cand) {
  const int64_t i = a.item_row[j];
  if (i < 0 || i >= a.f) return false;
  const int64_t c = j - a.item_ptr[i];
  const int64_t v = a.front[i];
  if (c < 0 || v < 0 || v >= a.N) return false;
  int64_t rb, re;
  row_range(a.indptr, a.nnz, v, &rb, &re);
  if (!item_slots(rb, re, c, kChunk, beg, end)) return false;
  *cand = a.cand_ptr[i] + c * kChunk;
  return true;
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void trv_claim_kernel(Args a) {
  const int64_t j = block_linear() * kWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (j >= a.bound) return;  // the whole wave
  int64_t beg = 0, end = 0, cand = 0;
  if (!item_range(a, j, &beg, &end, &cand)) return;
  for (int64_t s = beg; s < end; s += 64 * kUnroll) {
    int32_t d[kUnroll];
    bool open[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t slot = s + u * 64 + lane;
      d[u] = slot < end ? a.indices[slot] : -1;
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      // a target outside [0, N) is not followed
      open[u] = static_cast<uint32_t>(d[u]) < static_cast<uint64_t>(a.N);
      if (MODE == kBfs) open[u] = open[u] && a.visited[d[u]] == 0;
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      if (!open[u]) continue;
      const u64 c = static_cast<u64>(cand + (s - beg) + u * 64 + lane);
      if (MODE == kBfs) {
        atomicMin(a.claim + d[u], c);
      } else {
        atomicAdd(reinterpret_cast<u64*>(a.remain + d[u]), ~u64(0));  // minus one
        atomicMax(a.claim + d[u], static_cast<u64>(a.key_base) + c);
      }
    }
  }
}

// FILL = false: item_cnt[j] = winners of item j (0 past the end).
// FILL = true: the winners are written from item_base[j] on.
template <int MODE, bool FILL>
__global__ __launch_bounds__(kThreads) void trv_walk_kernel(Args a) {
  const int64_t j = block_linear() * kWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (j >= a.bound) return;  // the whole wave
  int64_t beg = 0, end = 0, cand = 0;
  if (!item_range(a, j, &beg, &end, &cand)) {
    if (!FILL && lane == 0) a.item_cnt[j] = 0;
    return;
  }
  int64_t out = FILL ? a.item_base[j] : 0;
  int64_t next_deg = 0;
  const u64 below = lanes_below(lane);
  for (int64_t s = beg; s < end; s += 64 * kUnroll) {
    int32_t d[kUnroll];
    bool ok[kUnroll], free_[kUnroll];
    u64 owner[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t slot = s + u * 64 + lane;
      d[u] = slot < end ? a.indices[slot] : -1;
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      ok[u] = static_cast<uint32_t>(d[u]) < static_cast<uint64_t>(a.N);
      free_[u] = false;
      owner[u] = 0;
      if (ok[u]) {
        free_[u] = MODE == kBfs ? a.visited[d[u]] == 0 : a.remain[d[u]] == 0;
        owner[u] = a.claim[d[u]];
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      u64 key = static_cast<u64>(cand + (s - beg) + u * 64 + lane);
      if (MODE == kTopo) key += static_cast<u64>(a.key_base);
      const bool win = ok[u] && free_[u] && owner[u] == key;
      const u64 mask = __ballot(win);
      if constexpr (FILL) {
        const int64_t o = out + __popcll(mask & below);
        if (win && o < a.cap) {
          a.next[o] = d[u];
          if (a.next_edge) a.next_edge[o] = a.eid[s + u * 64 + lane];
          int64_t b, e;
          row_range(a.indptr, a.nnz, d[u], &b, &e);
          next_deg += e - b;
        }
      }
      out += __popcll(mask);
    }
  }
  if (FILL) wave_add(next_deg, a.status + 1);
  if (!FILL && lane == 0) a.item_cnt[j] = out;
}

__global__ void trv_status_kernel(Args a) {
  a.status[0] = a.item_base[a.bound];
  a.status[3] = a.item_ptr[a.f];
}

// Level zero of the topological traversal: remain[v] is v's degree in the
// opposite CSR, and the nodes of degree zero are compacted in ascending id by
// flag, scan of the per-wave counts and ballot.
struct TopoArgs {
  int64_t N, nnz, waves;
  const int64_t* indptr;
  const int64_t* opposite;
  int64_t* remain;
  int64_t* wave_cnt;
  int64_t* wave_base;
  int64_t* out;
  int64_t* status;
};

__global__ __launch_bounds__(kThreads) void topo_flag_kernel(TopoArgs t) {
  const int64_t i = block_linear() * kThreads + threadIdx.x;
  bool zero = false;
  if (i < t.N) {
    const int64_t r = t.opposite[i + 1] - t.opposite[i];
    t.remain[i] = r < 0 ? 0 : r;
    zero = r <= 0;
  }
  const u64 mask = __ballot(zero);
  const int64_t w = i >> 6;
  if ((threadIdx.x & 63) == 0 && w < t.waves) t.wave_cnt[w] = __popcll(mask);
}

__global__ __launch_bounds__(kThreads) void topo_place_kernel(TopoArgs t) {
  const int64_t i = block_linear() * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool zero = i < t.N && t.remain[i] == 0;
  const u64 mask = __ballot(zero);
  int64_t deg = 0;
  if (zero) {
    const int64_t pos = t.wave_base[i >> 6] + __popcll(mask & lanes_below(lane));
    if (pos < t.N) t.out[pos] = i;
    int64_t b, e;
    row_range(t.indptr, t.nnz, i, &b, &e);
    deg = e - b;
  }
  wave_add(deg, t.status + 1);
}

__global__ void topo_status_kernel(TopoArgs t) { t.status[0] = t.wave_base[t.waves]; }

struct TopoLayout {
  int64_t waves, wave_cnt, wave_base, scan, scan_len, total;
  explicit TopoLayout(int64_t N) {
    waves = (N + 63) / 64;
    Carve c;
    wave_cnt = c.take(waves * 8);
    wave_base = c.take((waves + 1) * 8);
    scan_len = round256(int64_t(waves > 0 ? scan_bytes_i64(waves) : 0));
    scan = c.take(scan_len);
    total = c.off;
  }
};

void check_graph(int64_t N, int64_t nnz) {
  DGLHIP_CHECK(N >= 0 && nnz >= 0, "negative size");
  DGLHIP_CHECK(N < (int64_t(1) << 31), "node ids are 32-bit in the CSR");
}

constexpr const char* kNoCapture =
    "a traversal reads every frontier's size on the host and cannot be captured";

template <int MODE>
void launch_level(const Args& a, const Layout& L, char* ws, hipStream_t stream) {
  hipLaunchKernelGGL(trv_reset_kernel, dim3(1), dim3(64), 0, stream, a);
  char* scan_ws = ws + L.scan;
  hipLaunchKernelGGL(trv_degree_kernel, grid_1d((a.f + kThreads - 1) / kThreads), dim3(kThreads),
                     0, stream, a);
  HIP_CALL(hipGetLastError());
  scan_i64(scan_ws, L.scan_len, a.deg, a.cand_ptr + 1, a.f, stream);
  scan_i64(scan_ws, L.scan_len, a.nit, a.item_ptr + 1, a.f, stream);
  const dim3 per_item = grid_1d((a.bound + kWaves - 1) / kWaves);
  launch_item_rows(a.f, a.bound, a.item_ptr, a.item_row, stream);
  hipLaunchKernelGGL((trv_claim_kernel<MODE>), per_item, dim3(kThreads), 0, stream, a);
  hipLaunchKernelGGL((trv_walk_kernel<MODE, false>), per_item, dim3(kThreads), 0, stream, a);
  HIP_CALL(hipGetLastError());
  scan_i64(scan_ws, L.scan_len, a.item_cnt, a.item_base + 1, a.bound, stream);
  hipLaunchKernelGGL((trv_walk_kernel<MODE, true>), per_item, dim3(kThreads), 0, stream, a);
  hipLaunchKernelGGL(trv_status_kernel, dim3(1), dim3(1), 0, stream, a);
  HIP_CALL(hipGetLastError());
}

}  // namespace

}  // namespace dglhip

using namespace dglhip;

extern "C" {

int64_t dglhip_traversal_level_workspace_bytes(int64_t frontier_len, int64_t num_candidates) {
  try {
    DGLHIP_CHECK(frontier_len >= 1 && frontier_len < (int64_t(1) << 31) && num_candidates >= 0,
                 "bad frontier of " << frontier_len << " rows, " << num_candidates << " slots");
    return Layout(frontier_len, num_candidates).total;
  } catch (const std::exception& e) {
    set_last_error(e.what());
    return -1;
  }
}

int64_t dglhip_topological_init_workspace_bytes(int64_t num_nodes) {
  try {
    check_graph(num_nodes, 0);
    return TopoLayout(num_nodes).total;
  } catch (const std::exception& e) {
    set_last_error(e.what());
    return -1;
  }
}

int dglhip_bfs_init_device(int64_t num_nodes, int64_t nnz, const int64_t* indptr,
                           const int64_t* source, int64_t num_sources, uint64_t* claim,
                           uint8_t* visited, int64_t* status, void* stream_) {
  API_BEGIN();
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  check_graph(num_nodes, nnz);
  check_not_capturing(stream, kNoCapture);
  DGLHIP_CHECK(num_sources >= 0 && num_sources < (int64_t(1) << 31),
               "bad number of sources " << num_sources);
  DGLHIP_CHECK(indptr && status && (num_sources == 0 || source) &&
                   (num_nodes == 0 || (claim && visited)),
               "null pointer argument");
  HIP_CALL(hipMemsetAsync(status, 0, 4 * sizeof(int64_t), stream));
  if (num_nodes > 0) {
    HIP_CALL(hipMemsetAsync(claim, 0xFF, size_t(num_nodes) * sizeof(uint64_t), stream));
    HIP_CALL(hipMemsetAsync(visited, 0, size_t(num_nodes), stream));
  }
  if (num_sources > 0) {
    hipLaunchKernelGGL(trv_source_kernel, grid_1d((num_sources + kThreads - 1) / kThreads),
                       dim3(kThreads), 0, stream, num_nodes, nnz, num_sources, indptr, source,
                       status);
    HIP_CALL(hipGetLastError());
  }
  API_END();
}

int dglhip_topological_init_device(int64_t num_nodes, int64_t nnz, const int64_t* indptr,
                                   const int64_t* opposite_indptr, uint64_t* claim,
                                   int64_t* remain, int64_t* out, void* workspace,
                                   int64_t workspace_bytes, int64_t* status, void* stream_) {
  API_BEGIN();
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  check_graph(num_nodes, nnz);
  check_not_capturing(stream, kNoCapture);
  DGLHIP_CHECK(status, "null pointer argument");
  HIP_CALL(hipMemsetAsync(status, 0, 4 * sizeof(int64_t), stream));
  if (num_nodes == 0) return 0;
  DGLHIP_CHECK(indptr && opposite_indptr && claim && remain && out && workspace,
               "null pointer argument");
  const TopoLayout L(num_nodes);
  check_workspace(workspace_bytes, L.total);
  char* ws = static_cast<char*>(workspace);
  TopoArgs t;
  t.N = num_nodes; t.nnz = nnz; t.waves = L.waves;
  t.indptr = indptr; t.opposite = opposite_indptr; t.remain = remain;
  t.wave_cnt = reinterpret_cast<int64_t*>(ws + L.wave_cnt);
  t.wave_base = reinterpret_cast<int64_t*>(ws + L.wave_base);
  t.out = out; t.status = status;
  HIP_CALL(hipMemsetAsync(claim, 0, size_t(num_nodes) * sizeof(uint64_t), stream));
  HIP_CALL(hipMemsetAsync(t.wave_base, 0, sizeof(int64_t), stream));
  const dim3 grid = grid_1d((num_nodes + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(topo_flag_kernel, grid, dim3(kThreads), 0, stream, t);
  HIP_CALL(hipGetLastError());
  scan_i64(ws + L.scan, L.scan_len, t.wave_cnt, t.wave_base + 1, L.waves, stream);
  hipLaunchKernelGGL(topo_place_kernel, grid, dim3(kThreads), 0, stream, t);
  hipLaunchKernelGGL(topo_status_kernel, dim3(1), dim3(1), 0, stream, t);
  HIP_CALL(hipGetLastError());
  API_END();
}

int dglhip_traversal_level_device(int mode, int64_t num_nodes, int64_t nnz, const int64_t* indptr,
                                  const int32_t* indices, const int64_t* eid,
                                  const int64_t* frontier, int64_t frontier_len,
                                  int64_t num_candidates, int64_t key_base, uint64_t* claim,
                                  uint8_t* visited, int64_t* remain, int64_t* next,
                                  int64_t* next_edge, int64_t next_capacity, void* workspace,
                                  int64_t workspace_bytes, int64_t* status, void* stream_) {
  API_BEGIN();
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  check_graph(num_nodes, nnz);
  check_not_capturing(stream, kNoCapture);
  DGLHIP_CHECK(mode == kBfs || mode == kTopo, "unknown traversal mode " << mode);
  DGLHIP_CHECK(num_nodes >= 1 && frontier_len >= 1 && frontier_len < (int64_t(1) << 31) &&
                   num_candidates >= 0 && key_base >= 0 && next_capacity >= 0,
               "bad level: " << frontier_len << " rows, " << num_candidates << " slots");
  DGLHIP_CHECK(indptr && frontier && claim && status && workspace &&
                   (mode == kBfs ? visited != nullptr : remain != nullptr) &&
                   (nnz == 0 || indices) && (next_capacity == 0 || next) &&
                   (!next_edge || eid),
               "null pointer argument");
  const Layout L(frontier_len, num_candidates);
  check_workspace(workspace_bytes, L.total);
  char* ws = static_cast<char*>(workspace);
  Args a;
  a.N = num_nodes; a.nnz = nnz; a.f = frontier_len; a.bound = L.bound;
  a.key_base = key_base; a.cap = next_capacity;
  a.indptr = indptr; a.indices = indices; a.eid = eid; a.front = frontier;
  a.claim = reinterpret_cast<u64*>(claim);
  a.visited = mode == kBfs ? visited : nullptr;
  a.remain = mode == kTopo ? remain : nullptr;
  a.deg = reinterpret_cast<int64_t*>(ws + L.deg);
  a.nit = reinterpret_cast<int64_t*>(ws + L.nit);
  a.cand_ptr = reinterpret_cast<int64_t*>(ws + L.cand_ptr);
  a.item_ptr = reinterpret_cast<int64_t*>(ws + L.item_ptr);
  a.item_row = reinterpret_cast<int32_t*>(ws + L.item_row);
  a.item_cnt = reinterpret_cast<int64_t*>(ws + L.item_cnt);
  a.item_base = reinterpret_cast<int64_t*>(ws + L.item_base);
  a.next = next; a.next_edge = next_edge; a.status = status;
  if (mode == kBfs) launch_level<kBfs>(a, L, ws, stream);
  else launch_level<kTopo>(a, L, ws, stream);
  API_END();
}

}  // extern "C"
