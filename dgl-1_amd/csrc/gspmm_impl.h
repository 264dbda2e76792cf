// The generic g-SpMM reducers (sum / mean / max, every message and
// edge-feature layout) and their launch logic, over the row primitives of
// gspmm_rows.h. Included by gspmm.hip (the C-ABI, which only declares the two
// dispatch_me overloads) and by gspmm_inst.hip, which is compiled once per
// (message, edge layout) pair (-DGSPMM_INST_MSG / -DGSPMM_INST_EM, see the
// Makefile) and instantiates them, so the kernel variants build in parallel
// translation units. The blocked schedule's two- and four-items-per-wave
// kernels are a unit of their own, gspmm_items.hip.
// Design notes: gspmm.hip header and DESIGN.md §4.1.
#pragma once
#include <initializer_list>

#include "gspmm_rows.h"

namespace dglhip {

// Sum-reduce kernel (also MEAN). GROUP lanes per work item, VEC floats per
// lane. A work item is a whole row (CHUNKED = false: item i = row_order[i]),
// or a slot range [chunk_beg[i], chunk_end[i]) whose sum goes to out[i, :]
// (CHUNKED = true). With ACCUM the chain continues from the value already in
// out[i, :] (segment-by-segment evaluation of one sequential chain); with
// MEAN and ACCUM on whole rows the row's mean is added to the value in
// out[i, :] (out + mean: a sum of two terms, the same bits either way round).
template <int VEC, int GROUP, int UNROLL, int MSG, int EM, bool MEAN, bool CHUNKED,
          bool ACCUM, int POL = POL_DEFAULT, bool BUF = false, int RP = 0>
__global__ __launch_bounds__(256) void gspmm_sum_kernel(
    int64_t num_items, int64_t F, int64_t elen, int64_t ldu,
    const int64_t* __restrict__ indptr,
    const int32_t* __restrict__ indices, const int64_t* __restrict__ eid,
    const float* __restrict__ ufeat, const float* __restrict__ efeat,
    float* __restrict__ out, const int32_t* __restrict__ row_order,
    const int64_t* __restrict__ chunk_beg, const int64_t* __restrict__ chunk_end) {
  typedef typename Vec<VEC>::T V;
  constexpr int ITEMS_PER_WAVE = 64 / GROUP;
  const int lane = threadIdx.x & 63;
  // wave index is uniform; make that explicit so slot data goes through SGPRs
  const int64_t wave =
      block_linear() * (blockDim.x >> 6) +
      __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int64_t it = wave * ITEMS_PER_WAVE + (GROUP == 64 ? 0 : lane / GROUP);
  if (it >= num_items) return;
  const int gl = GROUP == 64 ? lane : (lane % GROUP);
  int64_t row, beg, end;
  if (CHUNKED) {
    // item it: slots [chunk_beg[it], chunk_end[it]) into row row_order[it]
    // (the blocked schedule's items), or into partial row it (heavy-row
    // chunks, row ranges); the three loads are independent
    row = row_order ? row_order[it] : it;
    if (GROUP == 64) row = __builtin_amdgcn_readfirstlane(static_cast<int>(row));
    beg = chunk_beg[it];
    end = chunk_end[it];
  } else {
    row = row_order ? row_order[it] : it;
    if (GROUP == 64) row = __builtin_amdgcn_readfirstlane(static_cast<int>(row));
    beg = indptr[row];
    end = indptr[row + 1];
  }
  for (int64_t f0 = int64_t(gl) * VEC; f0 < F; f0 += int64_t(GROUP) * VEC) {
    const int64_t eoff = EM == EM_HEAD ? f0 / (F / elen) : (EM == EM_FULL ? f0 : 0);
    constexpr bool ADD_MEAN = MEAN && ACCUM && !CHUNKED;
    V acc = (ACCUM && !ADD_MEAN) ? load_out<VEC, RP>(out + row * F, f0) : Vec<VEC>::zero();
    if (copies_u(MSG) || eid != nullptr)  // uniform branch
      acc = reduce_range<VEC, UNROLL, MSG, EM, true, BUF && GROUP == 64>(
          acc, beg, end, ldu, F, f0, elen, eoff, indices, eid, ufeat, efeat);
    else
      acc = reduce_range<VEC, UNROLL, MSG, EM, false>(acc, beg, end, ldu, F, f0, elen, eoff, indices,
                                                      eid, ufeat, efeat);
    if (!CHUNKED && MEAN && end - beg > 1)
      acc = acc / Vec<VEC>::splat(static_cast<float>(end - beg));
    if (ADD_MEAN) acc = ldv<VEC>(out + row * F + f0) + acc;
    if (RP) store_out<VEC, RP>(out + row * F, f0, acc);
    else store_row<VEC, POL>(out + row * F + f0, acc);
  }
}

// Combine the chunk partials of each heavy row in chunk order:
// out[row] = ((p0 + p1) + p2) + ... (deterministic), then MEAN scaling; with
// ACCUM the row's running value comes first: out[row] = ((out[row] + p0) + p1) ...;
// with MEAN and ACCUM the mean is added to it: out[row] + (p0 + p1 + ...) / deg
template <bool MEAN, bool ACCUM>
__global__ __launch_bounds__(256) void gspmm_combine_kernel(
    int64_t num_heavy, int64_t F, const int64_t* __restrict__ indptr,
    const int32_t* __restrict__ heavy_rows, const int64_t* __restrict__ heavy_chunk_ptr,
    const float* __restrict__ partial, float* __restrict__ out) {
  const int64_t wave = block_linear() * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (wave >= num_heavy) return;
  const int lane = threadIdx.x & 63;
  const int64_t row = heavy_rows[wave];
  const int64_t c0 = heavy_chunk_ptr[wave], c1 = heavy_chunk_ptr[wave + 1];
  const float deg = static_cast<float>(indptr[row + 1] - indptr[row]);
  for (int64_t f = lane; f < F; f += 64) {
    float acc = (ACCUM && !MEAN) ? out[row * F + f] + partial[c0 * F + f] : partial[c0 * F + f];
    for (int64_t c = c0 + 1; c < c1; ++c) acc += partial[c * F + f];
    if (MEAN && deg > 1.0f) acc = acc / deg;
    if (MEAN && ACCUM) acc = out[row * F + f] + acc;
    out[row * F + f] = acc;
  }
}

// Max-reduce kernel with argmax slot: first slot wins ties (a strict running
// max over the mailbox, seeded with the first message), and a NaN message is
// taken like a larger one and then kept (torch.max: the row's first NaN wins,
// value and argmax; segment_reduce.hip's max_step is the same rule); 0 / -1
// for rows without slots. Same lane mapping as the sum kernel (GROUP lanes
// per row, VEC features per lane, UNROLL gathers in flight); the compares
// then run slot by slot in CSR order, so the argmax is the one the sequential
// reduction picks. A NaN running value is never replaced, so a row continued
// from an earlier source block (prev) keeps the earlier block's NaN.
// The rule is "best is not NaN, and x is greater or NaN"; !(x <= best) is
// "greater or unordered", and the mask AND keeps it two compares without the
// per-element branches a short-circuit && / || compiles to.
__device__ __forceinline__ bool max_takes(float x, float best) {
  return (best == best) & !(x <= best);
}

template <int VEC, int UNROLL, int MSG, int EM, bool USE_EID>
__device__ __forceinline__ void max_row(int64_t row, int gl, int group, int64_t beg,
                                        int64_t end, int64_t F, int64_t elen,
                                        const int32_t* __restrict__ indices,
                                        const int64_t* __restrict__ eid,
                                        const float* __restrict__ ufeat,
                                        const float* __restrict__ efeat,
                                        float* __restrict__ out, int64_t* __restrict__ arg_out,
                                        bool prev = false) {
  typedef typename Vec<VEC>::T V;
  auto message = [](const SlotLoad<VEC, MSG, EM>& s) -> V {
    if (copies_u(MSG)) return s.u;
    if (MSG == DGLHIP_MSG_COPY_E) return s.e;
    return s.u * s.e;
  };
  auto edge = [&](int64_t k) -> int64_t {
    return copies_u(MSG) ? 0 : (USE_EID ? eid[k] : k);
  };
  for (int64_t f0 = int64_t(gl) * VEC; f0 < F; f0 += int64_t(group) * VEC) {
    const int64_t eoff = EM == EM_HEAD ? f0 / (F / elen) : (EM == EM_FULL ? f0 : 0);
    V best = Vec<VEC>::zero();
    int64_t arg[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) arg[i] = -1;
    int64_t k = beg;
    if (prev) {  // the row's earlier slots (a previous source block): continue from them
      best = ldv<VEC>(out + row * F + f0);
#pragma unroll
      for (int i = 0; i < VEC; ++i) arg[i] = arg_out ? arg_out[row * F + f0 + i] : -1;
    } else if (k < end) {
      SlotLoad<VEC, MSG, EM> s;
      s.load(ufeat, efeat, F, F, f0, elen, eoff, indices[k], edge(k));
      best = message(s);
#pragma unroll
      for (int i = 0; i < VEC; ++i) arg[i] = k;
      ++k;
    }
    for (; k + UNROLL <= end; k += UNROLL) {
      SlotLoad<VEC, MSG, EM> s[UNROLL];
#pragma unroll
      for (int j = 0; j < UNROLL; ++j)
        s[j].load(ufeat, efeat, F, F, f0, elen, eoff, indices[k + j], edge(k + j));
#pragma unroll
      for (int j = 0; j < UNROLL; ++j) {
        const V x = message(s[j]);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const float xi = reinterpret_cast<const float*>(&x)[i];
          float& bi = reinterpret_cast<float*>(&best)[i];
          if (max_takes(xi, bi)) { bi = xi; arg[i] = k + j; }
        }
      }
    }
    const int64_t rem = end - k;  // the last < UNROLL slots: one predicated batch
    if (rem > 0) {
      SlotLoad<VEC, MSG, EM> s[UNROLL];
#pragma unroll
      for (int j = 0; j < UNROLL - 1; ++j)
        if (j < rem) s[j].load(ufeat, efeat, F, F, f0, elen, eoff, indices[k + j], edge(k + j));
#pragma unroll
      for (int j = 0; j < UNROLL - 1; ++j) {
        if (j < rem) {
          const V x = message(s[j]);
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            const float xi = reinterpret_cast<const float*>(&x)[i];
            float& bi = reinterpret_cast<float*>(&best)[i];
            if (max_takes(xi, bi)) { bi = xi; arg[i] = k + j; }
          }
        }
      }
    }
    stv<VEC>(out + row * F + f0, best);
    if (arg_out) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) arg_out[row * F + f0 + i] = arg[i];
    }
  }
}

template <int VEC, int GROUP, int UNROLL, int MSG, int EM>
__global__ __launch_bounds__(256) void gspmm_max_kernel(
    int64_t num_rows, int64_t F, int64_t elen, const int64_t* __restrict__ indptr,
    const int32_t* __restrict__ indices, const int64_t* __restrict__ eid,
    const float* __restrict__ ufeat, const float* __restrict__ efeat,
    float* __restrict__ out, int64_t* __restrict__ arg_out,
    const int32_t* __restrict__ row_order, const int64_t* __restrict__ row_beg,
    const int64_t* __restrict__ row_end, int accumulate) {
  constexpr int ITEMS_PER_WAVE = 64 / GROUP;
  const int lane = threadIdx.x & 63;
  const int64_t wave =
      block_linear() * (blockDim.x >> 6) +
      __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int64_t it = wave * ITEMS_PER_WAVE + (GROUP == 64 ? 0 : lane / GROUP);
  if (it >= num_rows) return;
  const int gl = GROUP == 64 ? lane : (lane % GROUP);
  int64_t row = row_order ? row_order[it] : it;
  if (GROUP == 64) row = __builtin_amdgcn_readfirstlane(static_cast<int>(row));
  // row ranges (source-blocked schedule): the row's slots [row_beg, row_end)
  // of this block; with accumulate, continue from the earlier blocks' max
  const int64_t rs = indptr[row];
  const int64_t beg = row_beg ? row_beg[row] : rs;
  const int64_t end = row_end ? row_end[row] : indptr[row + 1];
  if (accumulate && beg == end) return;  // nothing new: the row keeps its value
  const bool prev = accumulate && beg > rs;
  if (copies_u(MSG) || eid != nullptr)  // uniform branch
    max_row<VEC, UNROLL, MSG, EM, true>(row, gl, GROUP, beg, end, F, elen, indices, eid, ufeat,
                                        efeat, out, arg_out, prev);
  else
    max_row<VEC, UNROLL, MSG, EM, false>(row, gl, GROUP, beg, end, F, elen, indices, eid,
                                         ufeat, efeat, out, arg_out, prev);
}

// ---------------------------------------------------------------------------
// Dispatch
// ---------------------------------------------------------------------------
// Widest per-lane vector the row length and every feature pointer allow.
static inline int pick_vec(int64_t F, std::initializer_list<const void*> ptrs) {
  auto aligned = [&](int bytes) {
    for (const void* p : ptrs)
      if (p && (reinterpret_cast<uintptr_t>(p) % bytes) != 0) return false;
    return true;
  };
  // no VEC 4: at F=256 one 1-KB row per wave instruction (8 gathers
  // in flight) ran 16.3 ms against 15.7 ms for two VEC-2 passes with 16 in
  // flight (profiles/r01/feat_sweep_reddit.json, Reddit-shaped graph)
  if (F % 2 == 0 && F >= 4 && aligned(8)) return 2;
  return 1;
}

static inline int pick_group(int64_t F, int vec) {
  const int64_t lanes = (F + vec - 1) / vec;
  int g = 1;
  while (g < lanes && g < 64) g <<= 1;
  return g;
}

// Rows of 16..64 floats take a whole wave each (idle lanes) rather than
// sharing one: the slot stream is then wave-uniform (column ids through the
// scalar cache) instead of a per-lane index load ahead of every gather.
// profiles/r01/feat_sweep_reddit.json, Reddit-shaped graph: F=16 2.18 -> 1.73 ms, F=32
// 2.12 -> 1.74 ms, F=64 level.
static inline void one_row_per_wave(int64_t F, int& vec, int& group) {
  if (group < 64 && F >= 16) {
    vec = 1;
    group = 64;
  }
}

struct SumLaunch {
  int64_t num_items, F, elen;
  const int64_t* indptr;
  const int32_t* indices;
  const int64_t* eid;
  const float* ufeat;
  const float* efeat;
  float* out;
  const int32_t* row_order;
  const int64_t* chunk_beg;  // non-null: chunked launch (partials to `out`)
  const int64_t* chunk_end;
  bool accumulate;           // continue each item's chain from the value in `out`
  bool nt_out = false;       // non-temporal output stores (see stream_output)
  int64_t ldu = 0;           // ufeat row stride in elements (0: F)
};

template <int VEC, int GROUP, int MSG, int EM, bool MEAN>
static inline void launch_sum(const SumLaunch& a, hipStream_t stream) {
  // 16 row gathers in flight per lane group: measured +22% over 8 on HBM-bound
  // RMAT, neutral on the MALL-resident Reddit table
  constexpr int UNROLL = 16;
  constexpr int ITEMS_PER_BLOCK = 4 * (64 / GROUP);
  const int64_t blocks = (a.num_items + ITEMS_PER_BLOCK - 1) / ITEMS_PER_BLOCK;
  DGLHIP_CHECK(blocks <= 0x7fffffff, "grid too large: " << blocks);
  if (blocks == 0) return;
  const bool chunked = a.chunk_beg != nullptr;
  // every instantiation has one signature: choose the kernel, then launch it
  auto kernel = gspmm_sum_kernel<VEC, GROUP, UNROLL, MSG, EM, MEAN, false, false>;
  if (chunked && a.accumulate)
    kernel = gspmm_sum_kernel<VEC, GROUP, UNROLL, MSG, EM, MEAN, true, true>;
  else if (chunked)
    kernel = gspmm_sum_kernel<VEC, GROUP, UNROLL, MSG, EM, MEAN, true, false>;
  else if (a.accumulate)
    kernel = gspmm_sum_kernel<VEC, GROUP, UNROLL, MSG, EM, MEAN, false, true>;
  // copy_u + sum with a whole wave of two-float lanes per row (F = 128 and
  // wider): the one shape with an output policy, buffer-descriptor gathers
  // and a running-row policy
  constexpr bool POL_OK = MSG == DGLHIP_MSG_COPY_U && VEC == 2 && GROUP == 64 && !MEAN;
  if constexpr (POL_OK) {
    if (chunked && a.row_order && !a.nt_out) {
      // the blocked schedule's items (item rows given; heavy-row chunk and
      // row-range launches keep the generic kernels: r04 ADVICE). Row gathers
      // through per-row buffer descriptors (the row base in SGPRs, one lane
      // offset for all 16: 42 instead of 70 VGPRs, 8 waves per SIMD instead of
      // 7; Reddit-shaped headline 3.74 -> 3.61 ms, same bits); the running
      // rows under RP 2, the first launch, which only stores, under RP 4.
      // (Rows of 128 floats go two or four items to a wave where
      // gspmm_items.hip's gate says so, and never come here.)
      if (a.accumulate)
        kernel = gspmm_sum_kernel<VEC, GROUP, UNROLL, MSG, EM, false, true, true, POL_DEFAULT,
                                  true, 2>;
      else
        kernel = gspmm_sum_kernel<VEC, GROUP, UNROLL, MSG, EM, false, true, false, POL_DEFAULT,
                                  true, 4>;
    } else if (a.nt_out && !a.accumulate) {
      // an output past twice the Infinity Cache (stream_output)
      if (chunked)
        kernel = gspmm_sum_kernel<VEC, GROUP, UNROLL, MSG, EM, false, true, false, POL_NT_OUT>;
      else
        kernel = gspmm_sum_kernel<VEC, GROUP, UNROLL, MSG, EM, false, false, false, POL_NT_OUT>;
    }
  }
  timed_launch(stream, [&] {
    hipLaunchKernelGGL(kernel, grid_1d(blocks), dim3(256), 0, stream, a.num_items, a.F, a.elen,
                       a.ldu ? a.ldu : a.F, a.indptr, a.indices, a.eid, a.ufeat, a.efeat, a.out,
                       a.row_order, a.chunk_beg, a.chunk_end);
  });
}

template <int MSG, int EM, bool MEAN>
static inline void dispatch_sum_shape(const SumLaunch& a, hipStream_t stream) {
  const int64_t F = a.F;
  int vec = pick_vec(F, {a.ufeat, EM == EM_FULL ? a.efeat : nullptr, a.out});
  // per-head weights: a lane's VEC features must stay inside one head
  while (EM == EM_HEAD && vec > 1 && (F / a.elen) % vec != 0) vec >>= 1;
  int group = pick_group(F, vec);
  one_row_per_wave(F, vec, group);
#define DGLHIP_CASE(V, G)                                  \
  if (vec == V && group == G) {                            \
    launch_sum<V, G, MSG, EM, MEAN>(a, stream);            \
    return;                                                \
  }
  DGLHIP_CASE(2, 64) DGLHIP_CASE(2, 32) DGLHIP_CASE(2, 16) DGLHIP_CASE(2, 8)
  DGLHIP_CASE(2, 4) DGLHIP_CASE(2, 2)
  DGLHIP_CASE(1, 64) DGLHIP_CASE(1, 32) DGLHIP_CASE(1, 16) DGLHIP_CASE(1, 8)
  DGLHIP_CASE(1, 4) DGLHIP_CASE(1, 2) DGLHIP_CASE(1, 1)
#undef DGLHIP_CASE
  DGLHIP_CHECK(false, "no kernel for F=" << F << " vec=" << vec << " group=" << group);
}

static inline int edge_mode(int64_t elen, int64_t F) {
  return elen == F ? EM_FULL : (elen == 1 ? EM_SCALAR : EM_HEAD);
}


struct MaxLaunch {
  int64_t num_rows, F, elen;
  const int64_t* indptr;
  const int32_t* indices;
  const int64_t* eid;
  const float* ufeat;
  const float* efeat;
  float* out;
  int64_t* arg_out;
  const int32_t* row_order;
  const int64_t* row_beg = nullptr;  // row ranges (NULL: whole rows)
  const int64_t* row_end = nullptr;
  int accumulate = 0;
};


template <int MSG, int EM>
static inline void dispatch_max_shape(const MaxLaunch& a, hipStream_t stream) {
  const int64_t F = a.F;
  int vec = pick_vec(F, {a.ufeat, EM == EM_FULL ? a.efeat : nullptr, a.out});
  while (EM == EM_HEAD && vec > 1 && (F / a.elen) % vec != 0) vec >>= 1;
  int group = pick_group(F, vec);
  one_row_per_wave(F, vec, group);
#define DGLHIP_CASE(V, G)                                                            \
  if (vec == V && group == G) {                                                      \
    constexpr int ITEMS_PER_BLOCK = 4 * (64 / G);                                    \
    const int64_t blocks = (a.num_rows + ITEMS_PER_BLOCK - 1) / ITEMS_PER_BLOCK;     \
    DGLHIP_CHECK(blocks <= 0x7fffffff, "grid too large: " << blocks);                \
    timed_launch(stream, [&] {                                                       \
      hipLaunchKernelGGL((gspmm_max_kernel<V, G, 8, MSG, EM>),                       \
                         grid_1d(blocks), dim3(256), 0, stream,  \
                         a.num_rows, a.F, a.elen, a.indptr, a.indices, a.eid,        \
                         a.ufeat, a.efeat, a.out, a.arg_out, a.row_order, a.row_beg, \
                         a.row_end, a.accumulate);                                   \
    });                                                                              \
    return;                                                                          \
  }
  DGLHIP_CASE(2, 64) DGLHIP_CASE(2, 32) DGLHIP_CASE(2, 16) DGLHIP_CASE(2, 8)
  DGLHIP_CASE(2, 4) DGLHIP_CASE(2, 2)
  DGLHIP_CASE(1, 64) DGLHIP_CASE(1, 32) DGLHIP_CASE(1, 16) DGLHIP_CASE(1, 8)
  DGLHIP_CASE(1, 4) DGLHIP_CASE(1, 2) DGLHIP_CASE(1, 1)
#undef DGLHIP_CASE
  DGLHIP_CHECK(false, "no max kernel for F=" << F << " vec=" << vec << " group=" << group);
}


// One (message, edge layout) pair of the sum/mean and max reducers. Defined
// only in gspmm_inst.hip, which explicitly instantiates it per pair.
template <int MSG, int EM>
void dispatch_me(bool mean, const SumLaunch& a, hipStream_t stream);
template <int MSG, int EM>
void dispatch_me(const MaxLaunch& a, hipStream_t stream);

#ifdef GSPMM_INST_MSG
template <int MSG, int EM>
void dispatch_me(bool mean, const SumLaunch& a, hipStream_t stream) {
  if (mean) dispatch_sum_shape<MSG, EM, true>(a, stream);
  else dispatch_sum_shape<MSG, EM, false>(a, stream);
}
template <int MSG, int EM>
void dispatch_me(const MaxLaunch& a, hipStream_t stream) {
  dispatch_max_shape<MSG, EM>(a, stream);
}
#endif

}  // namespace dglhip
