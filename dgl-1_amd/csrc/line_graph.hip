// Line graph of a mutable graph whose edge list and source-major CSR are on
// the device: DGLGraph.line_graph(ctx=a ROCm device).
//
// The answer is that of the native index's MutableGraph::line_graph
// (graph_index.cc; the reference's GraphOp::LineGraph, src/graph/graph_op.cc):
// for i = 0..E-1 with u = src[i], v = dst[i], the out-edges of v in slot
// (= edge-id) order are emitted as (i, eid[slot]), except those whose
// destination is u when not backtracking; the k-th emitted pair is line-graph
// edge k.
//
// Candidates: the concatenation over i of the slots of row dst[i];
// cand_ptr[i + 1] - cand_ptr[i] = outdeg(dst[i]) from one rocPRIM scan,
// K = cand_ptr[E] (int64: it passes 2^31 long before E does).
//
// Mapping: a lane owns a candidate, not a row. A tile of
// DGLHIP_LINE_GRAPH_TILE consecutive candidates is one work unit: kUnroll
// strides of 64 candidates, walked by one wave. The units are dealt to a
// fixed number of waves (segments(E), known from E alone so that the
// workspace is) in consecutive runs of ceil(units / segments): one unit per
// wave until there are more units than waves. Per unit the wave finds the
// edges of its first and last candidate by two wave-uniform binary searches
// in cand_ptr; every lane then searches only between those two for each of
// its kUnroll candidates, the kUnroll searches interleaved so that their loads
// are in flight together.
//
// Stage A (dglhip_line_graph_count_device), a fixed sequence of launches with
// no host round trip: degrees and validation, the scan, and when not
// backtracking the walk that ballots each stride's survivors and stores one
// count per wave, scanned in wave order. status = {M, K, invalid endpoints,
// units}. With backtracking candidate k is output k: M = K and nothing walks.
// The caller reads the status once, allocates, and runs
// Stage B (dglhip_line_graph_fill_device): the same walk; a lane's output
// position is its wave's scanned base, plus the survivors of the wave's
// earlier strides, plus the popcount of the ballot below its lane (k itself
// with backtracking). No atomic decides a position, every output element is
// written exactly once, a stride's stores go to consecutive addresses, and
// two runs give the same arrays.
#include "../../include/dgl_hip.h"
#include "compact.h"

namespace dglhip {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int64_t kTile = DGLHIP_LINE_GRAPH_TILE;
constexpr int kUnroll = int(kTile / 64);  // strides of a unit, searched together
constexpr int64_t kMaxSegments = 8192;    // 256 CUs x 32 resident waves

static_assert(kTile % 64 == 0 && kUnroll >= 1 && kUnroll <= 8, "a unit is a few whole strides");

// Waves the walk is dealt to: K <= E * E, so a small graph launches no more
// waves than it can have units.
int64_t segments(int64_t E) {
  const int64_t units = E * E / kTile + 1;  // E < 2^31
  return units < kMaxSegments ? units : kMaxSegments;
}

// The workspace both stages share (all sections 256-byte aligned).
struct Layout {
  int64_t segs;
  int64_t deg, cand_ptr, seg_cnt, seg_base, scan, scan_len, total;
  Layout(int64_t E) {
    segs = segments(E);
    Carve c;
    deg = c.take(E * 8);
    cand_ptr = c.take((E + 1) * 8);
    seg_cnt = c.take(segs * 8);
    seg_base = c.take((segs + 1) * 8);
    const size_t s0 = E > 0 ? scan_bytes_i64(E) : 0, s1 = scan_bytes_i64(segs);
    scan_len = round256(int64_t(s0 > s1 ? s0 : s1));
    scan = c.take(scan_len);
    total = c.off;
  }
};

struct Args {
  int64_t N, E, segs, m;
  const int64_t* src;
  const int64_t* dst;
  const int64_t* indptr;
  const int32_t* indices;
  const int64_t* eid;
  int64_t* deg;
  int64_t* cand_ptr;
  int64_t* seg_cnt;
  int64_t* seg_base;
  int64_t* status;
  int64_t* lsrc;
  int64_t* ldst;
};

// The slots of row v of the graph's own CSR (its nnz is E). The walk reads E
// through the argument struct here: its code is then the measured one.
__device__ __forceinline__ void row_range(const Args& a, int64_t v, int64_t* beg, int64_t* end) {
  dglhip::row_range(a.indptr, a.E, v, beg, end);
}

// deg[i] = outdeg(dst[i]); an edge with an endpoint outside [0, N) is counted
// and gets no candidates, so nothing ever follows it.
__global__ __launch_bounds__(kThreads) void lg_degree_kernel(Args a) {
  const int64_t i = block_linear() * kThreads + threadIdx.x;
  int64_t bad = 0;
  if (i < a.E) {
    const int64_t u = a.src[i], v = a.dst[i];
    const bool ub = u < 0 || u >= a.N, vb = v < 0 || v >= a.N;
    bad = int64_t(ub) + int64_t(vb);
    int64_t d = 0;
    if (!ub && !vb) {
      int64_t rb, re;
      row_range(a, v, &rb, &re);
      d = re - rb;
    }
    a.deg[i] = d;
  }
  wave_add(bad, a.status + 2);  // a validation counter, not a position
}

// BT: backtracking (every candidate is emitted, at its own index).
// FILL = false (never with BT): seg_cnt[w] = survivors of wave w's units.
// FILL = true: the survivors are written, from seg_base[w] on when !BT.
template <bool BT, bool FILL>
__global__ __launch_bounds__(kThreads) void lg_walk_kernel(Args a) {
  const int64_t w = block_linear() * kWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= a.segs) return;  // the whole wave
  int64_t K = a.cand_ptr[a.E];
  K = (K < 0 || a.E == 0) ? 0 : K;
  const int64_t units = (K + kTile - 1) / kTile;
  const int64_t per = (units + a.segs - 1) / a.segs;
  const int64_t ub = w * per;
  const int64_t ue = ub + per < units ? ub + per : units;
  int64_t out = (FILL && !BT) ? a.seg_base[w] : 0;
  const unsigned long long below = lanes_below(lane);
  for (int64_t unit = ub; unit < ue; ++unit) {
    const int64_t k0 = unit * kTile;
    const int64_t kend = k0 + kTile < K ? k0 + kTile : K;
    // wave-uniform: the edges that own the unit's first and last candidate
    // (edges without candidates share their successor's start and are skipped
    // by taking the last)
    const int64_t first = last_le(a.cand_ptr, k0, 0, a.E - 1);
    const int64_t last = last_le(a.cand_ptr, kend - 1, first, a.E - 1);
    int64_t lo[kUnroll], hi[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      lo[u] = first;
      hi[u] = k0 + u * 64 + lane < kend ? last : first;
    }
    // the kUnroll searches of a lane step together: their loads overlap
    bool open = true;
    while (open) {
      open = false;
      int64_t c[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) c[u] = a.cand_ptr[(lo[u] + hi[u] + 1) >> 1];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        if (lo[u] < hi[u]) {
          const int64_t mid = (lo[u] + hi[u] + 1) >> 1;
          if (c[u] <= k0 + u * 64 + lane) lo[u] = mid;
          else hi[u] = mid - 1;
          open = open || lo[u] < hi[u];
        }
      }
    }
    int64_t slot[kUnroll];
    bool keep[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t k = k0 + u * 64 + lane;
      const int64_t e = lo[u];
      keep[u] = false;
      slot[u] = 0;
      if (k < kend) {
        const int64_t v = a.dst[e];
        if (v >= 0 && v < a.N) {
          int64_t rb, re;
          row_range(a, v, &rb, &re);
          const int64_t s = rb + (k - a.cand_ptr[e]);
          if (s >= rb && s < re) {
            slot[u] = s;
            keep[u] = BT || int64_t(a.indices[s]) != a.src[e];
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      if constexpr (BT) {
        const int64_t k = k0 + u * 64 + lane;
        if (keep[u] && k < a.m) {
          a.lsrc[k] = lo[u];
          a.ldst[k] = a.eid[slot[u]];
        }
      } else {
        const unsigned long long mask = __ballot(keep[u]);
        if constexpr (FILL) {
          const int64_t o = out + __popcll(mask & below);
          if (keep[u] && o < a.m) {
            a.lsrc[o] = lo[u];
            a.ldst[o] = a.eid[slot[u]];
          }
        }
        out += __popcll(mask);
      }
    }
  }
  if (!FILL && lane == 0) a.seg_cnt[w] = out;
}

__global__ void lg_status_kernel(Args a, int backtracking) {
  int64_t K = a.cand_ptr[a.E];
  K = K < 0 ? 0 : K;
  a.status[0] = backtracking ? K : a.seg_base[a.segs];
  a.status[1] = K;
  a.status[3] = (K + kTile - 1) / kTile;
}

void check_sizes(int64_t N, int64_t E) {
  DGLHIP_CHECK(N >= 0 && E >= 0, "negative size");
  DGLHIP_CHECK(N < (int64_t(1) << 31) && E < (int64_t(1) << 31),
               "line_graph needs fewer than 2^31 nodes and edges (got " << N << " and " << E
               << "): line-graph node ids become 32-bit CSR column indices");
}

Args bind(const Layout& L, int64_t N, int64_t E, const int64_t* src, const int64_t* dst,
          const int64_t* indptr, const int32_t* indices, const int64_t* eid, void* workspace,
          int64_t* status) {
  char* ws = static_cast<char*>(workspace);
  Args a;
  a.N = N; a.E = E; a.segs = L.segs; a.m = 0;
  a.src = src; a.dst = dst; a.indptr = indptr; a.indices = indices; a.eid = eid;
  a.deg = reinterpret_cast<int64_t*>(ws + L.deg);
  a.cand_ptr = reinterpret_cast<int64_t*>(ws + L.cand_ptr);
  a.seg_cnt = reinterpret_cast<int64_t*>(ws + L.seg_cnt);
  a.seg_base = reinterpret_cast<int64_t*>(ws + L.seg_base);
  a.status = status;
  a.lsrc = a.ldst = nullptr;
  return a;
}

}  // namespace

}  // namespace dglhip

using namespace dglhip;

extern "C" {

int64_t dglhip_line_graph_workspace_bytes(int64_t num_nodes, int64_t num_edges) {
  try {
    check_sizes(num_nodes, num_edges);
    return Layout(num_edges).total;
  } catch (const std::exception& e) {
    set_last_error(e.what());
    return -1;
  }
}

int dglhip_line_graph_count_device(int64_t num_nodes, int64_t num_edges, const int64_t* src,
                                   const int64_t* dst, const int64_t* indptr,
                                   const int32_t* indices, int backtracking, void* workspace,
                                   int64_t workspace_bytes, int64_t* status, void* stream_) {
  API_BEGIN();
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  check_sizes(num_nodes, num_edges);
  check_not_capturing(stream, "the line graph reads its size on the host and cannot be captured");
  const int64_t E = num_edges;
  DGLHIP_CHECK(status && workspace && indptr && (E == 0 || (src && dst && indices)),
               "null pointer argument");
  const Layout L(E);
  check_workspace(workspace_bytes, L.total);
  const Args a = bind(L, num_nodes, E, src, dst, indptr, indices, nullptr, workspace, status);
  HIP_CALL(hipMemsetAsync(status, 0, 4 * sizeof(int64_t), stream));
  HIP_CALL(hipMemsetAsync(a.cand_ptr, 0, sizeof(int64_t), stream));
  HIP_CALL(hipMemsetAsync(a.seg_base, 0, sizeof(int64_t), stream));
  char* scan_ws = static_cast<char*>(workspace) + L.scan;
  if (E > 0) {
    hipLaunchKernelGGL(lg_degree_kernel, grid_1d((E + kThreads - 1) / kThreads), dim3(kThreads),
                       0, stream, a);
    HIP_CALL(hipGetLastError());
    scan_i64(scan_ws, L.scan_len, a.deg, a.cand_ptr + 1, E, stream);
  }
  if (!backtracking) {
    hipLaunchKernelGGL((lg_walk_kernel<false, false>), grid_1d((L.segs + kWaves - 1) / kWaves),
                       dim3(kThreads), 0, stream, a);
    HIP_CALL(hipGetLastError());
    scan_i64(scan_ws, L.scan_len, a.seg_cnt, a.seg_base + 1, L.segs, stream);
  }
  hipLaunchKernelGGL(lg_status_kernel, dim3(1), dim3(1), 0, stream, a, backtracking ? 1 : 0);
  HIP_CALL(hipGetLastError());
  API_END();
}

int dglhip_line_graph_fill_device(int64_t num_nodes, int64_t num_edges, const int64_t* src,
                                  const int64_t* dst, const int64_t* indptr,
                                  const int32_t* indices, const int64_t* eid, int backtracking,
                                  void* workspace, int64_t workspace_bytes, int64_t num_units,
                                  int64_t num_line_edges, int64_t* lsrc, int64_t* ldst,
                                  void* stream_) {
  API_BEGIN();
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  check_sizes(num_nodes, num_edges);
  DGLHIP_CHECK(num_units >= 0 && num_line_edges >= 0 &&
                   num_line_edges / kTile <= num_units,  // M <= K <= units * tile
               "bad line-graph size: " << num_line_edges << " edges in " << num_units
                                       << " units");
  if (num_line_edges == 0) return 0;
  DGLHIP_CHECK(num_units >= 1, "bad unit count " << num_units);
  DGLHIP_CHECK(workspace && src && dst && indptr && indices && eid && lsrc && ldst,
               "null pointer argument");
  const Layout L(num_edges);
  check_workspace(workspace_bytes, L.total);
  Args a = bind(L, num_nodes, num_edges, src, dst, indptr, indices, eid, workspace, nullptr);
  a.m = num_line_edges;
  a.lsrc = lsrc; a.ldst = ldst;
  // the waves that have units: the count stage's deal, ceil(units / segs) each
  const int64_t per = (num_units + L.segs - 1) / L.segs;
  int64_t waves = (num_units + per - 1) / per;
  waves = waves < L.segs ? waves : L.segs;
  const dim3 grid = grid_1d((waves + kWaves - 1) / kWaves);
  if (backtracking)
    hipLaunchKernelGGL((lg_walk_kernel<true, true>), grid, dim3(kThreads), 0, stream, a);
  else
    hipLaunchKernelGGL((lg_walk_kernel<false, true>), grid, dim3(kThreads), 0, stream, a);
  HIP_CALL(hipGetLastError());
  API_END();
}

}  // extern "C"
