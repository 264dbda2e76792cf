// Degree-bucketing schedule of a user-defined reduce function, built on the
// device from a receiver-major CSR that is already there: indptr
// int64[R + 1] and slot_msg int64[nnz], the message held by slot k (NULL:
// slot k holds message k). A CSR made by dglhip_coo_to_csr_device with
// ORDER_EID is such a one: a row's slots keep input order and eid is the
// input position, so no message is sorted again here.
//
// The answer is that of dglhip_degree_bucketing_host (host_graph.cc) for the
// message -> receiver array the CSR was built from, array for array: buckets
// are the distinct non-zero degrees ascending, rows ascend inside a bucket,
// a row's messages keep slot order. On top of it: the rows without messages
// (ascending) and merge_inv, the position of every row in nodes ++ zero_nodes.
//
// Stage A (dglhip_degree_buckets_count_device), a fixed sequence of launches
// with no host round trip:
//   1. key[r] = degree of row r through row_range (a bad indptr cannot index
//      outside the arrays), value r; rows with a degree are counted.
//   2. a stable rocPRIM radix sort of the pairs: position i holds the i-th
//      row by (degree, row id). The key bits come from nnz (a degree is at
//      most nnz), which the host knows. The rows without messages are the
//      first R - listed positions.
//   3. position i heads a bucket when its degree is non-zero and differs from
//      its predecessor's, and contributes ceil(deg / C) items of at most C =
//      DGLHIP_BUCKET_CHUNK slots: a hub row is not one wave's serial copy.
//      Three scans (rocPRIM): heads -> bucket numbers, degrees -> the end of
//      every position's run in the packed message list, items -> item_ptr.
//      Every item finds its position by the shared item-row search.
//   status = {buckets, listed rows, max degree, items}.
// The caller reads the status once, allocates the outputs, and runs
// Stage B (dglhip_degree_buckets_fill_device): one launch over positions for
// the bucket table, nodes, zero_nodes and merge_inv, one over items for
// msg_ids. Every output element has one writer whose value depends on the
// scans alone; the only atomic is the integer count of listed rows.
//
// Mapping: positions one per lane; items one per wave, four per 256-lane
// workgroup. Lane k of a stride copies slot beg + k to base + k, so the reads
// of slot_msg and the writes of msg_ids are whole 512-byte runs.
#include <rocprim/device/device_radix_sort.hpp>

#include "../../include/dgl_hip.h"
#include "compact.h"

namespace dglhip {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int64_t kChunk = DGLHIP_BUCKET_CHUNK;

// Items of R rows over nnz slots: the ceil(deg / C) sum to at most
// R + nnz / C.
int64_t item_bound(int64_t R, int64_t nnz) { return R + nnz / kChunk + 1; }

// Bits of a sort key: degrees lie in [0, nnz].
int key_bits(int64_t nnz) {
  int bits = 1;
  while (bits < 63 && (int64_t(1) << bits) <= nnz) ++bits;
  return bits;
}

size_t sort_bytes(int64_t R, int bits) {
  size_t bytes = 0;
  HIP_CALL(rocprim::radix_sort_pairs(nullptr, bytes, static_cast<const uint64_t*>(nullptr),
                                     static_cast<uint64_t*>(nullptr),
                                     static_cast<const int64_t*>(nullptr),
                                     static_cast<int64_t*>(nullptr), size_t(R), 0,
                                     unsigned(bits)));
  return bytes;
}

// The workspace both stages share (all sections 256-byte aligned). The sort
// writes to sections of its own (not a double buffer), so stage B knows where
// the sorted pairs are.
struct Layout {
  int64_t bound, bits;
  int64_t key, row, sdeg, srow, head, bucket, nit, item_ptr, msg_end, item_row, tmp, tmp_len,
      total;
  Layout(int64_t R, int64_t nnz) {
    bound = item_bound(R, nnz);
    bits = key_bits(nnz);
    Carve c;
    key = c.take(R * 8);
    row = c.take(R * 8);
    sdeg = c.take(R * 8);
    srow = c.take(R * 8);
    head = c.take(R * 8);
    bucket = c.take(R * 8);
    nit = c.take(R * 8);
    item_ptr = c.take((R + 1) * 8);
    msg_end = c.take(R * 8);
    item_row = c.take(bound * 4);
    const size_t s0 = R > 0 ? scan_bytes_i64(R) : 0, s1 = R > 0 ? sort_bytes(R, int(bits)) : 0;
    tmp_len = round256(int64_t(s0 > s1 ? s0 : s1));
    tmp = c.take(tmp_len);
    total = c.off;
  }
};

struct Args {
  int64_t R, nnz, nb, listed, items;
  const int64_t* indptr;
  const int64_t* slot_msg;
  uint64_t* key;
  int64_t* row;
  const uint64_t* sdeg;
  const int64_t* srow;
  int64_t* head;
  int64_t* bucket;
  int64_t* nit;
  int64_t* item_ptr;
  int64_t* msg_end;
  int32_t* item_row;
  int64_t* status;
  int64_t* bucket_deg;
  int64_t* bucket_node_ptr;
  int64_t* nodes;
  int64_t* zero_nodes;
  int64_t* msg_ids;
  int64_t* merge_inv;
};

__global__ __launch_bounds__(kThreads) void bkt_degree_kernel(Args a) {
  const int64_t r = block_linear() * kThreads + threadIdx.x;
  bool has = false;
  if (r < a.R) {
    int64_t beg, end;
    row_range(a.indptr, a.nnz, r, &beg, &end);
    a.key[r] = static_cast<uint64_t>(end - beg);
    a.row[r] = r;
    has = end > beg;
  }
  wave_count(has, a.status + 1);
}

__global__ __launch_bounds__(kThreads) void bkt_heads_kernel(Args a) {
  const int64_t i = block_linear() * kThreads + threadIdx.x;
  if (i >= a.R) return;
  const int64_t d = static_cast<int64_t>(a.sdeg[i]);
  a.head[i] = d > 0 && (i == 0 || static_cast<int64_t>(a.sdeg[i - 1]) != d) ? 1 : 0;
  a.nit[i] = (d + kChunk - 1) / kChunk;
}

__global__ void bkt_status_kernel(Args a) {
  a.status[0] = a.bucket[a.R - 1];
  a.status[2] = static_cast<int64_t>(a.sdeg[a.R - 1]);
  a.status[3] = a.item_ptr[a.R];
}

// Position i of the sorted rows: its entry of nodes or zero_nodes and of
// merge_inv, and its bucket's table entry when it heads one. The sizes the
// caller read bound every index.
__global__ __launch_bounds__(kThreads) void bkt_rows_kernel(Args a) {
  const int64_t i = block_linear() * kThreads + threadIdx.x;
  if (i == 0) a.bucket_node_ptr[a.nb] = a.listed;
  if (i >= a.R) return;
  const int64_t zeros = a.R - a.listed;
  const int64_t r = a.srow[i];
  if (r < 0 || r >= a.R) return;
  if (i < zeros) {
    a.zero_nodes[i] = r;
    a.merge_inv[r] = a.listed + i;
    return;
  }
  a.nodes[i - zeros] = r;
  a.merge_inv[r] = i - zeros;
  if (a.head[i]) {
    const int64_t b = a.bucket[i] - 1;
    if (b >= 0 && b < a.nb) {
      a.bucket_deg[b] = static_cast<int64_t>(a.sdeg[i]);
      a.bucket_node_ptr[b] = i - zeros;
    }
  }
}

// One wave per item: chunk c of the row at sorted position i, copied to its
// place in the packed message list.
__global__ __launch_bounds__(kThreads) void bkt_msgs_kernel(Args a) {
  const int64_t j = block_linear() * kWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (j >= a.items) return;  // the whole wave
  const int64_t i = a.item_row[j];
  if (i >= a.R) return;
  const int64_t c = j - a.item_ptr[i];
  const int64_t r = a.srow[i];
  if (c < 0 || r < 0 || r >= a.R) return;
  int64_t rb, re, beg, end;
  row_range(a.indptr, a.nnz, r, &rb, &re);
  if (!item_slots(rb, re, c, kChunk, &beg, &end)) return;
  const int64_t base = a.msg_end[i] - (re - rb) + c * kChunk;
  for (int64_t s = beg + lane; s < end; s += 64) {
    const int64_t o = base + (s - beg);
    if (o >= 0 && o < a.nnz) a.msg_ids[o] = a.slot_msg ? a.slot_msg[s] : s;
  }
}

void check_sizes(int64_t R, int64_t nnz) {
  DGLHIP_CHECK(R >= 0 && nnz >= 0, "negative size");
  DGLHIP_CHECK(R < (int64_t(1) << 31), "item rows are 32-bit positions");
}

Args bind(const Layout& L, int64_t R, int64_t nnz, const int64_t* indptr, void* workspace) {
  char* ws = static_cast<char*>(workspace);
  Args a = {};
  a.R = R; a.nnz = nnz;
  a.indptr = indptr;
  a.key = reinterpret_cast<uint64_t*>(ws + L.key);
  a.row = reinterpret_cast<int64_t*>(ws + L.row);
  a.sdeg = reinterpret_cast<const uint64_t*>(ws + L.sdeg);
  a.srow = reinterpret_cast<const int64_t*>(ws + L.srow);
  a.head = reinterpret_cast<int64_t*>(ws + L.head);
  a.bucket = reinterpret_cast<int64_t*>(ws + L.bucket);
  a.nit = reinterpret_cast<int64_t*>(ws + L.nit);
  a.item_ptr = reinterpret_cast<int64_t*>(ws + L.item_ptr);
  a.msg_end = reinterpret_cast<int64_t*>(ws + L.msg_end);
  a.item_row = reinterpret_cast<int32_t*>(ws + L.item_row);
  return a;
}

}  // namespace

}  // namespace dglhip

using namespace dglhip;

extern "C" {

int64_t dglhip_degree_buckets_workspace_bytes(int64_t num_rows, int64_t nnz) {
  try {
    check_sizes(num_rows, nnz);
    return Layout(num_rows, nnz).total;
  } catch (const std::exception& e) {
    set_last_error(e.what());
    return -1;
  }
}

int dglhip_degree_buckets_count_device(int64_t num_rows, int64_t nnz, const int64_t* indptr,
                                       void* workspace, int64_t workspace_bytes,
                                       int64_t* status, void* stream_) {
  API_BEGIN();
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  check_sizes(num_rows, nnz);
  check_not_capturing(stream,
                      "the degree buckets' sizes are read on the host and cannot be captured");
  DGLHIP_CHECK(status && workspace && indptr, "null pointer argument");
  const Layout L(num_rows, nnz);
  check_workspace(workspace_bytes, L.total);
  Args a = bind(L, num_rows, nnz, indptr, workspace);
  a.status = status;
  const int64_t R = num_rows;
  HIP_CALL(hipMemsetAsync(status, 0, 4 * sizeof(int64_t), stream));
  if (R == 0) return 0;
  HIP_CALL(hipMemsetAsync(a.item_ptr, 0, sizeof(int64_t), stream));
  const dim3 grid = grid_1d((R + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(bkt_degree_kernel, grid, dim3(kThreads), 0, stream, a);
  HIP_CALL(hipGetLastError());
  char* ws = static_cast<char*>(workspace);
  size_t temp = size_t(L.tmp_len);
  HIP_CALL(rocprim::radix_sort_pairs(ws + L.tmp, temp, static_cast<const uint64_t*>(a.key),
                                     reinterpret_cast<uint64_t*>(ws + L.sdeg),
                                     static_cast<const int64_t*>(a.row),
                                     reinterpret_cast<int64_t*>(ws + L.srow), size_t(R), 0,
                                     unsigned(L.bits), stream));
  hipLaunchKernelGGL(bkt_heads_kernel, grid, dim3(kThreads), 0, stream, a);
  HIP_CALL(hipGetLastError());
  scan_i64(ws + L.tmp, L.tmp_len, a.head, a.bucket, R, stream);
  scan_i64(ws + L.tmp, L.tmp_len, reinterpret_cast<const int64_t*>(a.sdeg), a.msg_end, R, stream);
  scan_i64(ws + L.tmp, L.tmp_len, a.nit, a.item_ptr + 1, R, stream);
  launch_item_rows(R, L.bound, a.item_ptr, a.item_row, stream);
  hipLaunchKernelGGL(bkt_status_kernel, dim3(1), dim3(1), 0, stream, a);
  HIP_CALL(hipGetLastError());
  API_END();
}

int dglhip_degree_buckets_fill_device(int64_t num_rows, int64_t nnz, const int64_t* indptr,
                                      const int64_t* slot_msg, void* workspace,
                                      int64_t workspace_bytes, int64_t num_buckets,
                                      int64_t listed, int64_t items, int64_t* bucket_deg,
                                      int64_t* bucket_node_ptr, int64_t* nodes,
                                      int64_t* zero_nodes, int64_t* msg_ids, int64_t* merge_inv,
                                      void* stream_) {
  API_BEGIN();
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  check_sizes(num_rows, nnz);
  DGLHIP_CHECK(listed >= 0 && listed <= num_rows, "bad count of listed rows " << listed);
  DGLHIP_CHECK(num_buckets >= 0 && num_buckets <= listed && (num_buckets > 0) == (listed > 0),
               "bad bucket count " << num_buckets);
  const Layout L(num_rows, nnz);
  DGLHIP_CHECK(items >= listed && items <= L.bound, "bad item count " << items);
  DGLHIP_CHECK(workspace && indptr && bucket_node_ptr, "null pointer argument");
  DGLHIP_CHECK((num_buckets == 0 || (bucket_deg && nodes && msg_ids)) &&
                   (num_rows == 0 || merge_inv) && (listed == num_rows || zero_nodes),
               "null pointer argument");
  check_workspace(workspace_bytes, L.total);
  Args a = bind(L, num_rows, nnz, indptr, workspace);
  a.slot_msg = slot_msg;
  a.nb = num_buckets; a.listed = listed; a.items = items;
  a.bucket_deg = bucket_deg; a.bucket_node_ptr = bucket_node_ptr;
  a.nodes = nodes; a.zero_nodes = zero_nodes; a.msg_ids = msg_ids; a.merge_inv = merge_inv;
  const int64_t n = num_rows > 0 ? num_rows : 1;  // bucket_node_ptr[nb] is written at R = 0 too
  hipLaunchKernelGGL(bkt_rows_kernel, grid_1d((n + kThreads - 1) / kThreads), dim3(kThreads), 0,
                     stream, a);
  if (items > 0)
    hipLaunchKernelGGL(bkt_msgs_kernel, grid_1d((items + kWaves - 1) / kWaves), dim3(kThreads),
                       0, stream, a);
  HIP_CALL(hipGetLastError());
  API_END();
}

}  // extern "C"
