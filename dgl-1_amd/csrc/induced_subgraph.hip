// Node-induced subgraph of a graph whose source-major CSR is on the device:
// DGLGraph.subgraph(nodes) for a node set given as a device tensor.
//
// The answer is that of the native index's MutableGraph::vertex_subgraph
// (graph_index.cc; the reference's Graph::VertexSubgraph, src/graph/graph.cc):
// for i = 0..n-1 the out-edges of sel[i] in slot order whose destination is
// selected, emitted as (i, newid[dst], eid[slot]); the k-th emitted edge is
// subgraph edge k.
//
// Stage A (dglhip_induced_subgraph_count_device), a fixed sequence of launches
// with no host round trip:
//   1. newid[N] = -1, then newid[sel[i]] = i for the ids in [0, N); the others
//      are counted as invalid and never used as an index.
//   2. position i is live when newid[sel[i]] == i; an in-range position that
//      is not live lost the scatter to a duplicate and is counted. A live
//      position contributes ceil(deg / C) items of at most C =
//      DGLHIP_SUBGRAPH_CHUNK slots; the item counts are scanned (rocPRIM) and
//      every item finds its position by the shared item-row search
//      (compact.h).
//   3. one wave per item counts the slots whose destination is selected; the
//      counts are scanned in item order, which is (position, chunk) order.
//   status = {edges, invalid ids, duplicate positions, items}.
// The caller reads the status once, allocates the outputs, and runs
// Stage B (dglhip_induced_subgraph_fill_device): the same walk; within a
// 64-slot stride a lane's output position is its item's scanned base, plus the
// survivors of the item's earlier strides, plus the popcount of the ballot
// below its lane. No atomic decides a position and every output element is
// written exactly once, so the arrays are the same on every run.
//
// Mapping: one wave per item, four items per 256-lane workgroup. Lane k of a
// stride reads slot base + k, so the index loads are whole 256-byte runs; the
// probes of newid are the random part, and four strides of indices are loaded
// before their four probes so that a wave keeps four probes in flight.
#include "../../include/dgl_hip.h"
#include "compact.h"

namespace dglhip {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int64_t kChunk = DGLHIP_SUBGRAPH_CHUNK;
constexpr int kUnroll = 4;  // strides whose probes are in flight together

static_assert(kChunk % (64 * kUnroll) == 0, "a chunk is a whole number of unrolled strides");

// Items of a selection of n positions over a CSR of nnz slots: the live
// positions are distinct rows, so their ceil(deg / C) sum to at most
// min(n, N) + nnz / C.
int64_t item_bound(int64_t N, int64_t n, int64_t nnz) {
  return (n < N ? n : N) + nnz / kChunk + 1;
}

// The workspace both stages share (all sections 256-byte aligned).
struct Layout {
  int64_t bound;
  int64_t newid, nit, item_ptr, item_row, item_cnt, item_base, scan, scan_len, total;
  Layout(int64_t N, int64_t n, int64_t nnz) {
    bound = item_bound(N, n, nnz);
    Carve c;
    newid = c.take(N * 4);
    nit = c.take(n * 8);
    item_ptr = c.take((n + 1) * 8);
    item_row = c.take(bound * 4);
    item_cnt = c.take(bound * 8);
    item_base = c.take((bound + 1) * 8);
    const size_t s0 = n > 0 ? scan_bytes_i64(n) : 0, s1 = scan_bytes_i64(bound);
    scan_len = round256(int64_t(s0 > s1 ? s0 : s1));
    scan = c.take(scan_len);
    total = c.off;
  }
};

struct Args {
  int64_t N, n, nnz, bound, m;
  const int64_t* indptr;
  const int32_t* indices;
  const int64_t* eid;
  const int64_t* sel;
  int32_t* newid;
  int64_t* nit;
  int64_t* item_ptr;
  int32_t* item_row;
  int64_t* item_cnt;
  int64_t* item_base;
  int64_t* status;
  int64_t* sub_src;
  int64_t* sub_dst;
  int64_t* parent_eid;
};

__global__ __launch_bounds__(kThreads) void sub_scatter_kernel(Args a) {
  const int64_t i = block_linear() * kThreads + threadIdx.x;
  bool bad = false;
  if (i < a.n) {
    const int64_t v = a.sel[i];
    if (v < 0 || v >= a.N) bad = true;
    else a.newid[v] = static_cast<int32_t>(i);  // duplicates: one of them stays
  }
  wave_count(bad, a.status + 1);
}

__global__ __launch_bounds__(kThreads) void sub_nitems_kernel(Args a) {
  const int64_t i = block_linear() * kThreads + threadIdx.x;
  bool dup = false;
  if (i < a.n) {
    const int64_t v = a.sel[i];
    int64_t items = 0;
    if (v >= 0 && v < a.N) {
      if (a.newid[v] == static_cast<int32_t>(i)) {
        int64_t beg, end;
        row_range(a.indptr, a.nnz, v, &beg, &end);
        items = (end - beg + kChunk - 1) / kChunk;
      } else {
        dup = true;
      }
    }
    a.nit[i] = items;
  }
  wave_count(dup, a.status + 2);
}

// The slots [beg, end) of item j and its position; false for an item past the
// end. Everything read here was bounded by the kernels above.
__device__ __forceinline__ bool item_range(const Args& a, int64_t j, int64_t* pos, int64_t* beg,
                                           int64_t* end) {
  const int64_t i = a.item_row[j];
  if (i >= a.n) return false;
  const int64_t c = j - a.item_ptr[i];
  const int64_t v = a.sel[i];
  if (c < 0 || v < 0 || v >= a.N) return false;
  int64_t rb, re;
  row_range(a.indptr, a.nnz, v, &rb, &re);
  *pos = i;
  return item_slots(rb, re, c, kChunk, beg, end);
}

// FILL = false: item_cnt[j] = survivors of item j (0 past the end).
// FILL = true: the survivors are written from item_base[j] on.
template <bool FILL>
__global__ __launch_bounds__(kThreads) void sub_walk_kernel(Args a) {
  const int64_t j = block_linear() * kWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (j >= a.bound) return;  // the whole wave
  int64_t pos = 0, beg = 0, end = 0;
  const bool live = item_range(a, j, &pos, &beg, &end);
  if (!live) {
    if (!FILL && lane == 0) a.item_cnt[j] = 0;
    return;
  }
  int64_t out = FILL ? a.item_base[j] : 0;
  const unsigned long long below = lanes_below(lane);
  for (int64_t s = beg; s < end; s += 64 * kUnroll) {
    int32_t d[kUnroll], p[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t slot = s + u * 64 + lane;
      d[u] = slot < end ? a.indices[slot] : -1;
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      // a destination outside [0, N) is not followed
      p[u] = static_cast<uint32_t>(d[u]) < static_cast<uint64_t>(a.N) ? a.newid[d[u]] : -1;
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const bool keep = p[u] >= 0;
      const unsigned long long mask = __ballot(keep);
      if constexpr (FILL) {
        const int64_t o = out + __popcll(mask & below);
        if (keep && o < a.m) {
          const int64_t slot = s + u * 64 + lane;
          a.sub_src[o] = pos;
          a.sub_dst[o] = p[u];
          a.parent_eid[o] = a.eid[slot];
        }
      }
      out += __popcll(mask);
    }
  }
  if (!FILL && lane == 0) a.item_cnt[j] = out;
}

__global__ void sub_status_kernel(Args a) {
  a.status[0] = a.item_base[a.bound];
  a.status[3] = a.item_ptr[a.n];
}

void check_sizes(int64_t N, int64_t n, int64_t nnz) {
  DGLHIP_CHECK(N >= 0 && n >= 0 && nnz >= 0, "negative size");
  DGLHIP_CHECK(N < (int64_t(1) << 31) && n < (int64_t(1) << 31),
               "node ids and positions are 32-bit in the membership map");
}

Args bind(const Layout& L, int64_t N, int64_t n, int64_t nnz, const int64_t* indptr,
          const int32_t* indices, const int64_t* eid, const int64_t* sel, void* workspace,
          int64_t* status) {
  char* ws = static_cast<char*>(workspace);
  Args a;
  a.N = N; a.n = n; a.nnz = nnz; a.bound = L.bound; a.m = 0;
  a.indptr = indptr; a.indices = indices; a.eid = eid; a.sel = sel;
  a.newid = reinterpret_cast<int32_t*>(ws + L.newid);
  a.nit = reinterpret_cast<int64_t*>(ws + L.nit);
  a.item_ptr = reinterpret_cast<int64_t*>(ws + L.item_ptr);
  a.item_row = reinterpret_cast<int32_t*>(ws + L.item_row);
  a.item_cnt = reinterpret_cast<int64_t*>(ws + L.item_cnt);
  a.item_base = reinterpret_cast<int64_t*>(ws + L.item_base);
  a.status = status;
  a.sub_src = a.sub_dst = a.parent_eid = nullptr;
  return a;
}

}  // namespace

}  // namespace dglhip

using namespace dglhip;

extern "C" {

int64_t dglhip_induced_subgraph_workspace_bytes(int64_t num_nodes, int64_t num_selected,
                                                int64_t nnz) {
  try {
    check_sizes(num_nodes, num_selected, nnz);
    return Layout(num_nodes, num_selected, nnz).total;
  } catch (const std::exception& e) {
    set_last_error(e.what());
    return -1;
  }
}

int dglhip_induced_subgraph_count_device(int64_t num_nodes, int64_t num_selected, int64_t nnz,
                                         const int64_t* indptr, const int32_t* indices,
                                         const int64_t* selected, void* workspace,
                                         int64_t workspace_bytes, int64_t* status,
                                         void* stream_) {
  API_BEGIN();
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  check_sizes(num_nodes, num_selected, nnz);
  check_not_capturing(stream,
                      "the induced subgraph reads its size on the host and cannot be captured");
  DGLHIP_CHECK(status && workspace && indptr && (nnz == 0 || indices) &&
                   (num_selected == 0 || selected),
               "null pointer argument");
  const Layout L(num_nodes, num_selected, nnz);
  check_workspace(workspace_bytes, L.total);
  const Args a = bind(L, num_nodes, num_selected, nnz, indptr, indices, nullptr, selected,
                      workspace, status);
  const int64_t n = num_selected;
  HIP_CALL(hipMemsetAsync(status, 0, 4 * sizeof(int64_t), stream));
  HIP_CALL(hipMemsetAsync(a.item_ptr, 0, sizeof(int64_t), stream));
  HIP_CALL(hipMemsetAsync(a.item_base, 0, sizeof(int64_t), stream));
  if (num_nodes > 0)
    HIP_CALL(hipMemsetAsync(a.newid, 0xFF, size_t(num_nodes) * sizeof(int32_t), stream));
  char* scan_ws = static_cast<char*>(workspace) + L.scan;
  if (n > 0) {
    const dim3 grid = grid_1d((n + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(sub_scatter_kernel, grid, dim3(kThreads), 0, stream, a);
    hipLaunchKernelGGL(sub_nitems_kernel, grid, dim3(kThreads), 0, stream, a);
    HIP_CALL(hipGetLastError());
    scan_i64(scan_ws, L.scan_len, a.nit, a.item_ptr + 1, n, stream);
  }
  launch_item_rows(n, L.bound, a.item_ptr, a.item_row, stream);
  hipLaunchKernelGGL((sub_walk_kernel<false>), grid_1d((L.bound + kWaves - 1) / kWaves),
                     dim3(kThreads), 0, stream, a);
  HIP_CALL(hipGetLastError());
  scan_i64(scan_ws, L.scan_len, a.item_cnt, a.item_base + 1, L.bound, stream);
  hipLaunchKernelGGL(sub_status_kernel, dim3(1), dim3(1), 0, stream, a);
  HIP_CALL(hipGetLastError());
  API_END();
}

int dglhip_induced_subgraph_fill_device(int64_t num_nodes, int64_t num_selected, int64_t nnz,
                                        const int64_t* indptr, const int32_t* indices,
                                        const int64_t* eid, const int64_t* selected,
                                        void* workspace, int64_t workspace_bytes,
                                        int64_t num_items, int64_t num_edges, int64_t* sub_src,
                                        int64_t* sub_dst, int64_t* parent_eid, void* stream_) {
  API_BEGIN();
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  check_sizes(num_nodes, num_selected, nnz);
  DGLHIP_CHECK(num_edges >= 0 && num_edges <= nnz, "bad edge count " << num_edges);
  if (num_edges == 0) return 0;
  DGLHIP_CHECK(workspace && indptr && indices && eid && selected && sub_src && sub_dst &&
                   parent_eid,
               "null pointer argument");
  const Layout L(num_nodes, num_selected, nnz);
  check_workspace(workspace_bytes, L.total);
  DGLHIP_CHECK(num_items >= 1 && num_items <= L.bound, "bad item count " << num_items);
  Args a = bind(L, num_nodes, num_selected, nnz, indptr, indices, eid, selected, workspace,
                nullptr);
  a.bound = num_items;  // the items the count stage found
  a.m = num_edges;
  a.sub_src = sub_src; a.sub_dst = sub_dst; a.parent_eid = parent_eid;
  hipLaunchKernelGGL((sub_walk_kernel<true>), grid_1d((num_items + kWaves - 1) / kWaves),
                     dim3(kThreads), 0, stream, a);
  HIP_CALL(hipGetLastError());
  API_END();
}

}  // extern "C"
