// Uniform neighbour sampling of a graph whose CSR is on the device: the device
// route of dgl.contrib.sampling.NeighborSampler for seeds given as a device
// tensor.
//
// The answer is that of the native index's sample_neighbors (graph_index.cc;
// the reference's ImmutableGraph::SampleSubgraph + CompactSubgraph) with the
// draw replaced by the stateless rule of sample_key.h: a row of d slots at
// fan-out k keeps every slot when d <= k, else the k positions with the
// smallest (key(seed, v, p), p), in ascending p. Seeds are layer 0 (a repeated
// seed counts once); a vertex first reached while layer h is expanded gets
// layer h + 1; vertices of layer < num_hops are expanded, each once. The
// subgraph's vertices are the visited ids ascending; its edges are the selected
// slots of the expanded vertices in ascending id, each row in ascending
// position. Everything is a function of (CSR, seeds, num_hops, k, seed): the
// host twin (neighbor_sample_host.cc) gives the same arrays bit for bit.
//
// Stages, the level loop being the caller's with one host read of `status`
// after the init call and after every hop:
//   init  layer[N] = -1; a seed in [0, N) claims layer 0 with a compare-and-
//         swap and the winners form frontier 0; the others are counted and
//         never used as an index.
//   hop h one wave per frontier vertex, four per 256-lane workgroup. The wave
//         computes its row's selection and claims every selected neighbour
//         with atomicCAS(&layer[nbr], -1, h + 1); the winners of a stride are
//         appended to the next frontier with one atomicAdd per wave. The order
//         of a frontier is arbitrary and nothing in the output depends on it;
//         the layers do not depend on who wins because hop h is complete
//         before hop h + 1 starts. The rows' min(d, k) are summed into the
//         status, so after the last hop the caller knows the vertex and the
//         edge count and the final stage needs no read.
//   final one scan over layer >= 0 gives every visited vertex its subgraph id
//         (vertices, layers); min(d, k) of the expanded ones is scanned into
//         each row's output base; the fill launch recomputes each expanded
//         row's selection and writes edge base + rank, rank from the ballots
//         below the lane. No atomic decides a position.
//
// Selecting the k smallest of d keys in a wave: an MSB-first binary radix
// select on the 64-bit key. Pass b counts the keys that agree with the prefix
// found so far and have bit b clear; the k-th smallest has bit b clear exactly
// when that count reaches the rank still wanted. After 64 passes the prefix is
// the k-th smallest key T and the rank left over is how many keys equal to T
// are taken, first positions first. Rows of at most DGLHIP_SAMPLE_REG_SLOTS
// slots keep their keys in registers (DGLHIP_SAMPLE_REG_SLOTS / 64 per lane)
// and count with ballots; longer rows recompute the hash in every pass and
// reduce per-lane counts once per pass. The cost does not depend on k and no
// row is too long. Only the selected slots' indices and eid are read: the key
// depends on the position, not on the neighbour.
//
// Weighted sampling (the *_weighted entry points) is the same machinery on the
// weighted key of sample_key.h, bits(E / node_weight[neighbour]): the hop and
// the fill kernel are templates on how a slot's key is obtained. That key
// reads the slot's neighbour and gathers its weight (after the id is known to
// lie in [0, N)), so every slot of a selected row is read. A row of up to
// DGLHIP_SAMPLE_REG_SLOTS slots computes each key once and emits from the
// registers it selected from; one of up to DGLHIP_SAMPLE_LDS_SLOTS computes
// each key once into the wave's own 8 KB slice of LDS and runs the passes and
// the emission from there; a longer row recomputes its keys, re-gathering
// indices and weights from L2, but selects a byte per pass with a histogram in
// that slice: eight passes and one more to emit. No row is too long.
#include "../../include/dgl_hip.h"
#include "compact.h"
#include "sample_key.h"

#include <rocprim/iterator/transform_iterator.hpp>

namespace dglhip {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRegSlots = DGLHIP_SAMPLE_REG_SLOTS;
constexpr int kRegKeys = kRegSlots / 64;
constexpr int kLdsSlots = DGLHIP_SAMPLE_LDS_SLOTS;

static_assert(kRegSlots % 64 == 0 && kRegKeys >= 1 && kRegKeys <= 8,
              "the register path holds a few whole strides of keys per lane");
static_assert(kLdsSlots >= kRegSlots && kWaves * kLdsSlots * 8 <= 64 * 1024,
              "a workgroup's staged keys fit its LDS");

using u64 = unsigned long long;

struct IsVisited {
  __host__ __device__ int32_t operator()(int32_t layer) const { return layer >= 0 ? 1 : 0; }
};

using VisitedIter = rocprim::transform_iterator<const int32_t*, IsVisited, int32_t>;

size_t scan_bytes_visited(int64_t len) {
  size_t bytes = 0;
  HIP_CALL(rocprim::inclusive_scan(nullptr, bytes,
                                   VisitedIter(static_cast<const int32_t*>(nullptr), IsVisited()),
                                   static_cast<int32_t*>(nullptr), size_t(len),
                                   rocprim::plus<int32_t>()));
  return bytes;
}

// The workspace of the final stage (all sections 256-byte aligned).
struct Layout {
  int64_t pos, cnt, base, scan, scan_len, total;
  Layout(int64_t N, int64_t V) {
    Carve c;
    pos = c.take(N * 4);
    cnt = c.take(V * 8);
    base = c.take((V + 1) * 8);
    const size_t s0 = N > 0 ? scan_bytes_visited(N) : 0, s1 = V > 0 ? scan_bytes_i64(V) : 0;
    scan_len = round256(int64_t(s0 > s1 ? s0 : s1));
    scan = c.take(scan_len);
    total = c.off;
  }
};

// How a slot's key is obtained. The uniform key is a hash of the position and
// is recomputed wherever it is needed. The weighted one reads the slot's
// neighbour and gathers its weight, only after the id is known to lie in
// [0, N): two dependent loads, a logarithm's worth of double arithmetic and a
// double division. So a weighted row computes each key once where it can
// (kKeepKeys): in registers up to kRegSlots slots, in the wave's LDS slice
// (stage) up to kLdsSlots, and only a longer row recomputes in every pass.
struct UniformKey {
  static constexpr bool kKeepKeys = false;
  uint64_t rb;
  __device__ __forceinline__ uint64_t operator()(int64_t p) const {
    return sample_slot_key(rb, p);
  }
};

struct WeightedKey {
  static constexpr bool kKeepKeys = true;
  uint64_t rb;
  const int32_t* row;  // indices + the row's first slot
  const float* weight;
  int64_t N;
  uint64_t* stage;  // kLdsSlots keys of LDS, this wave's own
  __device__ __forceinline__ uint64_t operator()(int64_t p) const {
    const int32_t nbr = row[p];
    uint32_t wbits = 0;  // a neighbour outside [0, N) is weightless
    if (static_cast<uint32_t>(nbr) < static_cast<uint64_t>(N)) wbits = __float_as_uint(weight[nbr]);
    return sample_weighted_slot_key(sample_slot_key(rb, p), wbits);
  }
};

// Keys a wave has staged in its LDS slice.
struct StagedKey {
  const uint64_t* key;
  __device__ __forceinline__ uint64_t operator()(int64_t p) const { return key[p]; }
};

// What a wave wrote to its own LDS slice is what its lanes read afterwards: a
// wave's LDS operations complete in order, so nothing is waited for; this
// only keeps the compiler from moving an access across.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// The keys of a row of d <= kRegSlots slots, slot r * 64 + lane in key[r]
// (0 past the row's end, where nothing is read).
template <typename KeyOf>
__device__ __forceinline__ void load_keys(const KeyOf& key_of, int64_t d, int lane,
                                          uint64_t (&key)[kRegKeys]) {
#pragma unroll
  for (int r = 0; r < kRegKeys; ++r) {
    const int64_t p = r * 64 + lane;
    key[r] = p < d ? key_of(p) : 0;
  }
}

// The k-th smallest (1-based, 1 <= k < d) of the d keys of a row in *thresh,
// and how many of the keys equal to it are taken in *take_eq: from the keys in
// registers (load_keys) ...
__device__ __forceinline__ void select_threshold_regs(const uint64_t (&key)[kRegKeys], int64_t d,
                                                      int64_t k, int lane, uint64_t* thresh,
                                                      int64_t* take_eq) {
  uint64_t prefix = 0;
  int64_t remaining = k;
  for (int bit = 63; bit >= 0; --bit) {
    int64_t zeros = 0;
#pragma unroll
    for (int r = 0; r < kRegKeys; ++r)
      zeros += __popcll(__ballot(r * 64 + lane < d && ((key[r] ^ prefix) >> bit) == 0));
    if (remaining > zeros) {
      prefix |= uint64_t(1) << bit;
      remaining -= zeros;
    }
  }
  *thresh = prefix;
  *take_eq = remaining;
}

// ... or, for a row of any length, asking key_of for every key in every pass.
// Every lane of the wave calls either with the same arguments and gets the
// same answer.
template <typename KeyOf>
__device__ __forceinline__ void select_threshold_passes(const KeyOf& key_of, int64_t d, int64_t k,
                                                        int lane, uint64_t* thresh,
                                                        int64_t* take_eq) {
  uint64_t prefix = 0;
  int64_t remaining = k;
  for (int bit = 63; bit >= 0; --bit) {
    int64_t zeros = 0;
    for (int64_t p = lane; p < d; p += 64) zeros += ((key_of(p) ^ prefix) >> bit) == 0 ? 1 : 0;
    zeros = wave_sum(zeros);
    if (remaining > zeros) {
      prefix |= uint64_t(1) << bit;
      remaining -= zeros;
    }
  }
  *thresh = prefix;
  *take_eq = remaining;
}

// One stride of the emission pass: the lane's slot p with its key against the
// threshold. out and eq_seen count the selected and the tied slots so far.
template <typename F>
__device__ __forceinline__ void emit_stride(bool in_row, uint64_t key, int64_t p, uint64_t thresh,
                                            int64_t take_eq, int lane, int64_t* out,
                                            int64_t* eq_seen, F&& f) {
  const u64 below = lanes_below(lane);
  const bool eq = in_row && key == thresh;
  const u64 eq_mask = __ballot(eq);
  const bool sel = in_row && (key < thresh ||
                              (eq && *eq_seen + __popcll(eq_mask & below) < take_eq));
  const u64 sel_mask = __ballot(sel);
  f(sel, p, *out + __popcll(sel_mask & below));
  *out += __popcll(sel_mask);
  *eq_seen += __popcll(eq_mask);
}

// The selection of a row of d > k >= 1 slots with its keys in registers.
template <typename KeyOf, typename F>
__device__ __forceinline__ void for_selected_regs(const KeyOf& key_of, int64_t d, int64_t k,
                                                  int lane, F&& f) {
  uint64_t key[kRegKeys];
  load_keys(key_of, d, lane, key);
  uint64_t thresh;
  int64_t take_eq, out = 0, eq_seen = 0;
  select_threshold_regs(key, d, k, lane, &thresh, &take_eq);
#pragma unroll
  for (int r = 0; r < kRegKeys; ++r) {
    const int64_t p = r * 64 + lane;
    if (r * 64 < d && out < k)  // the whole wave
      emit_stride(p < d, key[r], p, thresh, take_eq, lane, &out, &eq_seen, f);
  }
}

// The same threshold eight bits at a time, for a row whose keys are dear and
// fit nowhere: pass j computes every key once and counts, among the keys that
// agree with the prefix found so far, each value of the next byte in a 256-bin
// histogram (hist, 2 KB of the wave's own LDS); the byte of the k-th smallest
// is the first bin at which the running count reaches the rank still wanted.
// Eight passes over the keys where select_threshold_passes makes 64, the same
// answer: the prefix after byte j is that of the bit passes after bit 8 j.
template <typename KeyOf>
__device__ __forceinline__ void select_threshold_bytes(const KeyOf& key_of, int64_t d, int64_t k,
                                                       int lane, u64* hist, uint64_t* thresh,
                                                       int64_t* take_eq) {
  uint64_t prefix = 0;
  int64_t remaining = k;
  for (int shift = 56; shift >= 0; shift -= 8) {
    for (int b = lane; b < 256; b += 64) hist[b] = 0;
    wave_lds_sync();
    // (the bits above the byte: all of the key's but the low shift + 8, none at 56)
    const uint64_t above = shift == 56 ? 0 : ~uint64_t(0) << (shift + 8);
    for (int64_t p = lane; p < d; p += 64) {
      const uint64_t key = key_of(p);
      if (((key ^ prefix) & above) == 0) atomicAdd(hist + ((key >> shift) & 0xFF), u64(1));
    }
    wave_lds_sync();
    // lane l holds bins 4 l .. 4 l + 3; an inclusive scan of their sums finds
    // the one lane whose bins straddle the rank, and that lane the bin
    int64_t c[4], sum = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) sum += c[i] = static_cast<int64_t>(hist[lane * 4 + i]);
    long long incl = sum;
    for (int off = 1; off < 64; off <<= 1) {
      const long long up = __shfl_up(incl, off, 64);
      if (lane >= off) incl += up;
    }
    long long below = incl - sum;
    const bool mine = below < remaining && remaining <= incl;
    int digit = lane * 4;
    if (mine) {
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (digit == lane * 4 + i && below + c[i] < remaining) {
          below += c[i];
          ++digit;
        }
    }
    // (the keys that agree with the prefix are at least `remaining`: a lane has it)
    const int src = __ffsll(static_cast<long long>(__ballot(mine))) - 1;
    digit = __shfl(digit, src < 0 ? 0 : src, 64);
    below = __shfl(below, src < 0 ? 0 : src, 64);
    prefix |= uint64_t(digit & 0xFF) << shift;
    remaining -= below;
    wave_lds_sync();
  }
  *thresh = prefix;
  *take_eq = remaining;
}

// The emission pass with every key asked of key_of once more.
template <typename KeyOf, typename F>
__device__ __forceinline__ void emit_passes(const KeyOf& key_of, int64_t d, int64_t k, int lane,
                                            uint64_t thresh, int64_t take_eq, F&& f) {
  int64_t out = 0, eq_seen = 0;
  for (int64_t s = 0; s < d && out < k; s += 64) {
    const int64_t p = s + lane;
    emit_stride(p < d, p < d ? key_of(p) : 0, p, thresh, take_eq, lane, &out, &eq_seen, f);
  }
}

// Calls f(selected, p, rank) for the positions p = 0..d-1 of a row, a stride of
// 64 at a time and every lane of the wave in every call (so f may ballot);
// rank is the number of selected positions below p.
template <typename KeyOf, typename F>
__device__ __forceinline__ void for_selected(const KeyOf& key_of, int64_t d, int64_t k, int lane,
                                             F&& f) {
  if (k <= 0 || d <= 0) return;
  if (d <= k) {
    for (int64_t s = 0; s < d; s += 64) f(s + lane < d, s + lane, s + lane);
    return;
  }
  uint64_t thresh;
  int64_t take_eq;
  if constexpr (KeyOf::kKeepKeys) {
    if (d <= kRegSlots) {
      for_selected_regs(key_of, d, k, lane, f);
    } else if (d <= kLdsSlots) {
      for (int64_t p = lane; p < d; p += 64) key_of.stage[p] = key_of(p);
      wave_lds_sync();
      const StagedKey staged{key_of.stage};
      select_threshold_passes(staged, d, k, lane, &thresh, &take_eq);
      emit_passes(staged, d, k, lane, thresh, take_eq, f);
    } else {
      select_threshold_bytes(key_of, d, k, lane, reinterpret_cast<u64*>(key_of.stage), &thresh,
                             &take_eq);
      emit_passes(key_of, d, k, lane, thresh, take_eq, f);
    }
  } else {
    if (d <= kRegSlots) {
      uint64_t key[kRegKeys];
      load_keys(key_of, d, lane, key);
      select_threshold_regs(key, d, k, lane, &thresh, &take_eq);
    } else {
      select_threshold_passes(key_of, d, k, lane, &thresh, &take_eq);
    }
    emit_passes(key_of, d, k, lane, thresh, take_eq, f);
  }
}

// Appends the winners' ids to next[] behind *count: one atomicAdd per wave.
__device__ __forceinline__ void wave_append(bool win, int64_t id, int64_t* count, int64_t* next,
                                            int64_t cap, int lane) {
  const u64 mask = __ballot(win);
  if (mask == 0) return;  // the whole wave
  long long base = 0;
  if (lane == 0)
    base = static_cast<long long>(
        atomicAdd(reinterpret_cast<u64*>(count), static_cast<u64>(__popcll(mask))));
  base = __shfl(base, 0, 64);
  const int64_t pos = base + __popcll(mask & lanes_below(lane));
  if (win && pos < cap) next[pos] = id;
}

__global__ __launch_bounds__(kThreads) void ns_seed_kernel(int64_t N, int64_t n,
                                                           const int64_t* seeds, int32_t* layer,
                                                           int64_t* front, int64_t* status) {
  const int64_t i = block_linear() * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool bad = false, win = false;
  int64_t v = -1;
  if (i < n) {
    v = seeds[i];
    if (v < 0 || v >= N) bad = true;  // counted, never used as an index
    else win = atomicCAS(layer + v, -1, 0) == -1;
  }
  wave_count(bad, status + 1);
  wave_append(win, v, status, front, n, lane);
}

struct HopArgs {
  int64_t N, nnz, f, k, cap;
  int32_t next_layer;
  uint64_t seed;
  const int64_t* indptr;
  const int32_t* indices;
  const float* weight;  // the weighted kernels only
  const int64_t* front;
  int32_t* layer;
  int64_t* next;
  int64_t* status;
};

// The key source of the row of v, whose first slot is beg. Only the weighted
// kernels have the LDS slices (kLdsSlots keys per wave).
template <bool kWeighted, typename Args>
__device__ __forceinline__ auto row_keys(const Args& a, int64_t v, int64_t beg) {
  if constexpr (kWeighted) {
    __shared__ uint64_t stage[kWaves][kLdsSlots];
    return WeightedKey{sample_row_base(a.seed, v), a.indices + beg, a.weight, a.N,
                       stage[threadIdx.x >> 6]};
  } else {
    return UniformKey{sample_row_base(a.seed, v)};
  }
}

template <bool kWeighted>
__global__ __launch_bounds__(kThreads) void ns_hop_kernel(HopArgs a) {
  const int64_t i = block_linear() * kWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= a.f) return;  // the whole wave
  const int64_t v = a.front[i];
  if (v < 0 || v >= a.N) return;
  int64_t beg, end;
  row_range(a.indptr, a.nnz, v, &beg, &end);
  const int64_t d = end - beg;
  if (d == 0 || a.k <= 0) return;
  if (lane == 0)
    atomicAdd(reinterpret_cast<u64*>(a.status + 2), static_cast<u64>(d < a.k ? d : a.k));
  for_selected(row_keys<kWeighted>(a, v, beg), d, a.k, lane,
               [&](bool sel, int64_t p, int64_t) {
                 const int32_t nbr = sel ? a.indices[beg + p] : -1;
                 // a neighbour outside [0, N) is not followed
                 const bool ok = sel && static_cast<uint32_t>(nbr) < static_cast<uint64_t>(a.N);
                 const bool win = ok && atomicCAS(a.layer + nbr, -1, a.next_layer) == -1;
                 wave_append(win, nbr, a.status, a.next, a.cap, lane);
               });
}

struct FinalArgs {
  int64_t N, nnz, V, m, k;
  int32_t num_hops, in_dir;
  uint64_t seed;
  const int64_t* indptr;
  const int32_t* indices;
  const int64_t* eid;
  const float* weight;  // the weighted kernel only
  const int32_t* layer;
  const int32_t* pos;
  int64_t* cnt;
  int64_t* base;
  int64_t* vertices;
  int64_t* layers;
  int64_t* sub_src;
  int64_t* sub_dst;
  int64_t* parent_eid;
};

__global__ __launch_bounds__(kThreads) void ns_compact_kernel(FinalArgs a) {
  const int64_t v = block_linear() * kThreads + threadIdx.x;
  if (v >= a.N) return;
  const int32_t l = a.layer[v];
  if (l < 0) return;
  const int64_t i = int64_t(a.pos[v]) - 1;
  if (i < 0 || i >= a.V) return;
  int64_t c = 0;
  if (l < a.num_hops) {
    int64_t beg, end;
    row_range(a.indptr, a.nnz, v, &beg, &end);
    c = end - beg < a.k ? end - beg : a.k;
  }
  a.vertices[i] = v;
  a.layers[i] = l;
  a.cnt[i] = c;
}

template <bool kWeighted>
__global__ __launch_bounds__(kThreads) void ns_fill_kernel(FinalArgs a) {
  const int64_t i = block_linear() * kWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= a.V) return;  // the whole wave
  const int64_t v = a.vertices[i];
  if (v < 0 || v >= a.N || a.layers[i] >= a.num_hops) return;
  int64_t beg, end;
  row_range(a.indptr, a.nnz, v, &beg, &end);
  const int64_t out = a.base[i];
  for_selected(row_keys<kWeighted>(a, v, beg), end - beg, a.k, lane,
               [&](bool sel, int64_t p, int64_t rank) {
                 const int64_t o = out + rank;
                 if (!sel || o < 0 || o >= a.m) return;
                 const int32_t nbr = a.indices[beg + p];
                 int64_t nid = -1;  // a neighbour outside [0, N) was not followed
                 if (static_cast<uint32_t>(nbr) < static_cast<uint64_t>(a.N) && a.layer[nbr] >= 0)
                   nid = int64_t(a.pos[nbr]) - 1;
                 a.sub_src[o] = a.in_dir ? nid : i;
                 a.sub_dst[o] = a.in_dir ? i : nid;
                 a.parent_eid[o] = a.eid[beg + p];
               });
}

void check_sizes(int64_t N, int64_t nnz) {
  DGLHIP_CHECK(N >= 0 && nnz >= 0, "negative size");
  DGLHIP_CHECK(N < (int64_t(1) << 31), "node ids are 32-bit in the layer map");
}

constexpr const char* kNoCapture =
    "neighbour sampling reads every frontier's size on the host and cannot be captured";

// One hop, uniform or (weighted) by the node weights.
void launch_hop(int64_t num_nodes, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                const float* weight, bool weighted, const int64_t* frontier, int64_t frontier_len,
                int hop, int64_t fanout, uint64_t seed, int32_t* layer, int64_t* next,
                int64_t next_capacity, int64_t* status, hipStream_t stream) {
  check_sizes(num_nodes, nnz);
  check_not_capturing(stream, kNoCapture);
  DGLHIP_CHECK(num_nodes >= 1 && frontier_len >= 1 && frontier_len <= num_nodes && hop >= 0 &&
                   hop < (1 << 30) && fanout >= 0 && next_capacity >= 0,
               "bad hop " << hop << ": " << frontier_len << " rows, fan-out " << fanout);
  DGLHIP_CHECK(indptr && frontier && layer && status && (nnz == 0 || indices) &&
                   (next_capacity == 0 || next) && (!weighted || weight),
               "null pointer argument");
  HIP_CALL(hipMemsetAsync(status, 0, 4 * sizeof(int64_t), stream));
  HopArgs a;
  a.N = num_nodes; a.nnz = nnz; a.f = frontier_len; a.k = fanout; a.cap = next_capacity;
  a.next_layer = hop + 1; a.seed = seed;
  a.indptr = indptr; a.indices = indices; a.weight = weight; a.front = frontier;
  a.layer = layer; a.next = next; a.status = status;
  const dim3 grid = grid_1d((frontier_len + kWaves - 1) / kWaves);
  if (weighted) hipLaunchKernelGGL(ns_hop_kernel<true>, grid, dim3(kThreads), 0, stream, a);
  else hipLaunchKernelGGL(ns_hop_kernel<false>, grid, dim3(kThreads), 0, stream, a);
  HIP_CALL(hipGetLastError());
}

// The final stage; the fill launch repeats the hops' selection.
void launch_final(int64_t num_nodes, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                  const int64_t* eid, const float* weight, bool weighted, int in_direction,
                  int num_hops, int64_t fanout, uint64_t seed, const int32_t* layer,
                  int64_t num_vertices, int64_t num_edges, int64_t* vertices, int64_t* layers,
                  int64_t* sub_src, int64_t* sub_dst, int64_t* parent_eid, void* workspace,
                  int64_t workspace_bytes, hipStream_t stream) {
  check_sizes(num_nodes, nnz);
  DGLHIP_CHECK(num_vertices >= 0 && num_vertices <= num_nodes && num_edges >= 0 &&
                   num_edges <= nnz && num_hops >= 0 && fanout >= 0,
               "bad sample of " << num_vertices << " vertices, " << num_edges << " edges");
  if (num_vertices == 0) return;
  DGLHIP_CHECK(indptr && layer && vertices && layers && workspace && (!weighted || weight),
               "null pointer argument");
  DGLHIP_CHECK(num_edges == 0 || (indices && eid && sub_src && sub_dst && parent_eid),
               "null pointer argument");
  const Layout L(num_nodes, num_vertices);
  check_workspace(workspace_bytes, L.total);
  char* ws = static_cast<char*>(workspace);
  FinalArgs a;
  a.N = num_nodes; a.nnz = nnz; a.V = num_vertices; a.m = num_edges; a.k = fanout;
  a.num_hops = num_hops; a.in_dir = in_direction ? 1 : 0; a.seed = seed;
  a.indptr = indptr; a.indices = indices; a.eid = eid; a.weight = weight;
  a.layer = layer;
  int32_t* pos = reinterpret_cast<int32_t*>(ws + L.pos);
  a.pos = pos;
  a.cnt = reinterpret_cast<int64_t*>(ws + L.cnt);
  a.base = reinterpret_cast<int64_t*>(ws + L.base);
  a.vertices = vertices; a.layers = layers;
  a.sub_src = sub_src; a.sub_dst = sub_dst; a.parent_eid = parent_eid;
  size_t scan_len = size_t(L.scan_len);
  HIP_CALL(rocprim::inclusive_scan(ws + L.scan, scan_len, VisitedIter(layer, IsVisited()), pos,
                                   size_t(num_nodes), rocprim::plus<int32_t>(), stream));
  // a vertex count that is not the map's leaves rows unwritten: defined values
  HIP_CALL(hipMemsetAsync(a.cnt, 0, size_t(num_vertices) * sizeof(int64_t), stream));
  HIP_CALL(hipMemsetAsync(vertices, 0xFF, size_t(num_vertices) * sizeof(int64_t), stream));
  HIP_CALL(hipMemsetAsync(layers, 0xFF, size_t(num_vertices) * sizeof(int64_t), stream));
  HIP_CALL(hipMemsetAsync(a.base, 0, sizeof(int64_t), stream));
  hipLaunchKernelGGL(ns_compact_kernel, grid_1d((num_nodes + kThreads - 1) / kThreads),
                     dim3(kThreads), 0, stream, a);
  HIP_CALL(hipGetLastError());
  if (num_edges > 0) {
    scan_i64(ws + L.scan, L.scan_len, a.cnt, a.base + 1, num_vertices, stream);
    const dim3 grid = grid_1d((num_vertices + kWaves - 1) / kWaves);
    if (weighted) hipLaunchKernelGGL(ns_fill_kernel<true>, grid, dim3(kThreads), 0, stream, a);
    else hipLaunchKernelGGL(ns_fill_kernel<false>, grid, dim3(kThreads), 0, stream, a);
    HIP_CALL(hipGetLastError());
  }
}

}  // namespace

}  // namespace dglhip

using namespace dglhip;

extern "C" {

int64_t dglhip_neighbor_sample_workspace_bytes(int64_t num_nodes, int64_t num_vertices) {
  try {
    check_sizes(num_nodes, 0);
    DGLHIP_CHECK(num_vertices >= 0 && num_vertices <= num_nodes,
                 "bad vertex count " << num_vertices);
    return Layout(num_nodes, num_vertices).total;
  } catch (const std::exception& e) {
    set_last_error(e.what());
    return -1;
  }
}

int dglhip_neighbor_sample_init_device(int64_t num_nodes, const int64_t* seeds, int64_t num_seeds,
                                       int32_t* layer, int64_t* frontier, int64_t* status,
                                       void* stream_) {
  API_BEGIN();
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  check_sizes(num_nodes, 0);
  check_not_capturing(stream, kNoCapture);
  DGLHIP_CHECK(num_seeds >= 0 && num_seeds < (int64_t(1) << 31),
               "bad number of seeds " << num_seeds);
  DGLHIP_CHECK(status && (num_nodes == 0 || layer) && (num_seeds == 0 || (seeds && frontier)),
               "null pointer argument");
  HIP_CALL(hipMemsetAsync(status, 0, 4 * sizeof(int64_t), stream));
  if (num_nodes > 0)
    HIP_CALL(hipMemsetAsync(layer, 0xFF, size_t(num_nodes) * sizeof(int32_t), stream));
  if (num_seeds > 0) {
    hipLaunchKernelGGL(ns_seed_kernel, grid_1d((num_seeds + kThreads - 1) / kThreads),
                       dim3(kThreads), 0, stream, num_nodes, num_seeds, seeds, layer, frontier,
                       status);
    HIP_CALL(hipGetLastError());
  }
  API_END();
}

int dglhip_neighbor_sample_hop_device(int64_t num_nodes, int64_t nnz, const int64_t* indptr,
                                      const int32_t* indices, const int64_t* frontier,
                                      int64_t frontier_len, int hop, int64_t fanout, uint64_t seed,
                                      int32_t* layer, int64_t* next, int64_t next_capacity,
                                      int64_t* status, void* stream) {
  API_BEGIN();
  launch_hop(num_nodes, nnz, indptr, indices, nullptr, false, frontier, frontier_len, hop, fanout,
             seed, layer, next, next_capacity, status, static_cast<hipStream_t>(stream));
  API_END();
}

int dglhip_neighbor_sample_hop_device_weighted(int64_t num_nodes, int64_t nnz,
                                               const int64_t* indptr, const int32_t* indices,
                                               const float* node_weight, const int64_t* frontier,
                                               int64_t frontier_len, int hop, int64_t fanout,
                                               uint64_t seed, int32_t* layer, int64_t* next,
                                               int64_t next_capacity, int64_t* status,
                                               void* stream) {
  API_BEGIN();
  launch_hop(num_nodes, nnz, indptr, indices, node_weight, true, frontier, frontier_len, hop,
             fanout, seed, layer, next, next_capacity, status, static_cast<hipStream_t>(stream));
  API_END();
}

int dglhip_neighbor_sample_final_device(int64_t num_nodes, int64_t nnz, const int64_t* indptr,
                                        const int32_t* indices, const int64_t* eid,
                                        int in_direction, int num_hops, int64_t fanout,
                                        uint64_t seed, const int32_t* layer, int64_t num_vertices,
                                        int64_t num_edges, int64_t* vertices, int64_t* layers,
                                        int64_t* sub_src, int64_t* sub_dst, int64_t* parent_eid,
                                        void* workspace, int64_t workspace_bytes, void* stream) {
  API_BEGIN();
  launch_final(num_nodes, nnz, indptr, indices, eid, nullptr, false, in_direction, num_hops,
               fanout, seed, layer, num_vertices, num_edges, vertices, layers, sub_src, sub_dst,
               parent_eid, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
  API_END();
}

int dglhip_neighbor_sample_final_device_weighted(
    int64_t num_nodes, int64_t nnz, const int64_t* indptr, const int32_t* indices,
    const int64_t* eid, const float* node_weight, int in_direction, int num_hops, int64_t fanout,
    uint64_t seed, const int32_t* layer, int64_t num_vertices, int64_t num_edges,
    int64_t* vertices, int64_t* layers, int64_t* sub_src, int64_t* sub_dst, int64_t* parent_eid,
    void* workspace, int64_t workspace_bytes, void* stream) {
  API_BEGIN();
  launch_final(num_nodes, nnz, indptr, indices, eid, node_weight, true, in_direction, num_hops,
               fanout, seed, layer, num_vertices, num_edges, vertices, layers, sub_src, sub_dst,
               parent_eid, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
  API_END();
}

}  // extern "C"
