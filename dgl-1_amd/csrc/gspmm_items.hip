// The blocked schedule's item kernels for copy_u over fp32 rows of 128 floats:
// two items per wave (gspmm_items_pair_kernel) and four items per wave over a
// column half (gspmm_items_columns_kernel), the gate that picks between them
// and the generic one-item kernel (items_kernel, one pure function), their
// launches, and the items entries of the C-ABI. The kernels are templates on
// <DEPTH, ACCUM> only and use nothing of the generic reducers but the row
// primitives, so this unit does not see gspmm_impl.h: a launch the gate
// declines goes to gspmm.hip through gspmm_items_one.
// Design notes: DESIGN.md §4.1 "Two items per wave" and "Column halves".
#include <type_traits>

#include "gspmm_rows.h"
#include "spmm_plan.h"

namespace dglhip {

// Two items per wave: the blocked schedule's items for copy_u over fp32 rows
// of 128 floats (DESIGN.md §4.1 "Two items per wave"). Wave w takes items 2w
// (lanes 0-31) and 2w + 1 (lanes 32-63), each lane 4 consecutive floats, so
// one gather instruction fetches two whole source rows (1 KiB) and a short
// item's round trips carry twice the payload. Both items' column ids come
// from the scalar slot stream; a lane picks its half's id and gathers at a
// 32-bit byte offset from the table's one buffer descriptor (the launcher's
// gate: the table is shorter than 4 GiB). Each lane adds its item's slots in
// slot order from zero (ACCUM: from the running row): the chain of
// gspmm_sum_kernel, so the same bits. Slots that only the longer item has run
// with the shorter half's lanes switched off: nothing fetched, nothing added
// (not even a zero: -0.0 + 0.0 is +0.0). An odd item count ends on a wave whose upper half is off. Running
// rows as RP 2 (ACCUM) / RP 4 of the one-item kernel, 16 bytes per lane.
template <int DEPTH, bool ACCUM>
__global__ __launch_bounds__(256) void gspmm_items_pair_kernel(
    int64_t num_items, int64_t ldu, uint32_t table_bytes,
    const int32_t* __restrict__ indices, const float* __restrict__ ufeat,
    float* __restrict__ out, const int32_t* __restrict__ item_rows,
    const int64_t* __restrict__ item_ptr) {
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  constexpr int64_t F = 128;
  const int lane = threadIdx.x & 63;
  const int64_t wave =
      block_linear() * (blockDim.x >> 6) +
      __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int64_t i0 = wave * 2;
  if (i0 >= num_items) return;
  const bool two = i0 + 1 < num_items;  // uniform
  const bool hi = lane >= 32;
  // slots [b0, b1) into row r0, [b1, e1) into row r1
  const int64_t b0 = item_ptr[i0], b1 = item_ptr[i0 + 1];
  const int64_t e1 = two ? item_ptr[i0 + 2] : b1;
  const int64_t r0 = item_rows[i0];
  const int64_t r1 = two ? item_rows[i0 + 1] : r0;
  const int n0 = static_cast<int>(b1 - b0), n1 = static_cast<int>(e1 - b1);
  const int nmin = n0 < n1 ? n0 : n1, nmax = n0 < n1 ? n1 : n0;
  const int32_t* __restrict__ idx0 = indices + b0;
  const int32_t* __restrict__ idx1 = indices + b1;
  const uint32_t ld4 = static_cast<uint32_t>(ldu) * 4u;
  const uint32_t lane_off = static_cast<uint32_t>(lane & 31) * 16u;
  const __amdgpu_buffer_rsrc_t table = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(ufeat), 0, static_cast<int>(table_bytes), 0x00020000);
  const int64_t f0 = int64_t(lane & 31) * 4;
  float* const orow = out + (hi ? r1 : r0) * F;
  const bool owns = !hi || two;

  f32x4 acc = Vec<4>::zero();
  if (ACCUM && owns) acc = load_out<4, 2>(orow, f0);
  int k = 0;
  // both items have DEPTH slots left: every lane gathers, no predicate
#pragma unroll 1
  for (; k + DEPTH <= nmin; k += DEPTH) {
    u32x4 v[DEPTH];
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) {
      const uint32_t o0 = static_cast<uint32_t>(idx0[k + j]) * ld4;
      const uint32_t o1 = static_cast<uint32_t>(idx1[k + j]) * ld4;
      v[j] = __builtin_amdgcn_raw_buffer_load_b128(table, (hi ? o1 : o0) + lane_off, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) acc += *reinterpret_cast<const f32x4*>(&v[j]);
  }
  // the rest as predicated batches, every gather of a batch in flight
  // together. A lane whose item has no slot k + j is switched off for it: its
  // gather goes to an offset past the table, which the descriptor's range
  // check answers without a fetch, and the value is not added. The scalar
  // column loads stay inside the pair's slots (an ended item re-reads its
  // last id, an empty one the other item's).
  const int my_n = hi ? n1 : n0;
  const int32_t* __restrict__ tail0 = n0 > 0 ? idx0 : idx1;
  const int32_t* __restrict__ tail1 = n1 > 0 ? idx1 : idx0;
  const int last0 = n0 > 0 ? n0 - 1 : n1 - 1, last1 = n1 > 0 ? n1 - 1 : n0 - 1;
#pragma unroll 1
  for (; k < nmax; k += DEPTH) {
    const int rb = nmax - k;
    u32x4 v[DEPTH];
    int32_t c0[DEPTH], c1[DEPTH];
    // the batch's ids first, all in flight: one scalar round trip, not one
    // ahead of every gather (the empty asm keeps the compiler from sinking
    // each load to its use)
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) {
      c0[j] = tail0[k + j < last0 ? k + j : last0];
      c1[j] = tail1[k + j < last1 ? k + j : last1];
    }
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) asm volatile("" : "+s"(c0[j]), "+s"(c1[j]));
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) {
      if (j < rb) {  // uniform
        const uint32_t o0 = static_cast<uint32_t>(c0[j]) * ld4;
        const uint32_t o1 = static_cast<uint32_t>(c1[j]) * ld4;
        const uint32_t off = k + j < my_n ? (hi ? o1 : o0) + lane_off : 0xfffffff0u;
        v[j] = __builtin_amdgcn_raw_buffer_load_b128(table, off, 0, 0);
      }
    }
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) {
      if (j < rb) {
        const f32x4 sum = acc + *reinterpret_cast<const f32x4*>(&v[j]);
        acc = k + j < my_n ? sum : acc;
      }
    }
  }
  // one store per half: the row of a half is uniform, as store_out's
  // descriptor has to be
  if (!hi) store_out<4, ACCUM ? 2 : 4>(out + r0 * F, f0, acc);
  else if (two) store_out<4, ACCUM ? 2 : 4>(out + r1 * F, f0, acc);
}

// Lane j of every 16-lane row (a DPP row) handed to the whole row.
__device__ __forceinline__ uint32_t row_broadcast(uint32_t v, int j) {
  switch (j) {
#define DGLHIP_ROW_BCAST(J) \
  case J: return __builtin_amdgcn_update_dpp(0, v, 0x150 + J, 0xf, 0xf, true);
    DGLHIP_ROW_BCAST(0) DGLHIP_ROW_BCAST(1) DGLHIP_ROW_BCAST(2) DGLHIP_ROW_BCAST(3)
    DGLHIP_ROW_BCAST(4) DGLHIP_ROW_BCAST(5) DGLHIP_ROW_BCAST(6) DGLHIP_ROW_BCAST(7)
    DGLHIP_ROW_BCAST(8) DGLHIP_ROW_BCAST(9) DGLHIP_ROW_BCAST(10) DGLHIP_ROW_BCAST(11)
    DGLHIP_ROW_BCAST(12) DGLHIP_ROW_BCAST(13) DGLHIP_ROW_BCAST(14)
#undef DGLHIP_ROW_BCAST
    default: return __builtin_amdgcn_update_dpp(0, v, 0x15f, 0xf, 0xf, true);
  }
}

// Column halves: four items per wave over one half of the columns, for the
// launches of gspmm_items_pair_kernel (DESIGN.md §4.1 "Column halves"). A
// workgroup gathers only columns [64 * half, 64 * half + 64) of every source
// row, half = (block % 8) & 1: blocks b and b + 8 share an XCD, so each XCD's
// L2 holds one half of the launch's source slice instead of all of it. The
// label is for speed only: block b takes half b & 1 of item group b >> 1 (16
// items), a bijection onto all the work wherever the block runs. Wave w of a
// group takes items 4w .. 4w + 3, one per quarter (16 lanes, a DPP row, 16
// bytes per lane), so one gather instruction still fetches 1 KiB: four half
// rows. The column ids of a batch come from one vector load, lane 16t + j
// reading item t's slot k + j and turning it into the row's byte offset (or,
// past the item's end, an offset past the table, which the descriptor's
// range check answers without a fetch); a row broadcast hands slot j's offset
// to its quarter. Each lane adds its item's slots in slot order from zero
// (ACCUM: from the running row) and a switched-off lane adds nothing: the
// chain of gspmm_sum_kernel, the same bits.
// A wave's round trips other than its gathers are kept off its critical path
// (DESIGN.md §4.1 "Column halves", the wave schedule): the nine item records
// come in one scalar trip; the first ids leave ahead of the running row; the
// next batch's ids are loaded behind the gathers and looked at only after the
// batch's adds; the four rows leave in one store. Exactly 64 VGPRs (8 waves
// per SIMD): the kernel is compiled for that occupancy, check the resource
// usage for scratch after any change.
// A wave's ids in one trip (DESIGN.md §4.1 "Column halves", the id path): a
// wave whose four items have at most kItemsColumnsIdsCap slots together reads
// its slot range once, lane l slots 64c + l (coalesced dwords, up to four in
// flight together, the running row behind them), and writes the rows' byte
// offsets to its own region of LDS. A batch's offsets then come from one LDS
// read in place of the vector load, same lanes, same slots: no id load per
// batch, none behind the last one, and no vector round trip between two
// batches. The region is the wave's alone and LDS runs a wave's operations in
// order, so there is no workgroup barrier. A wave above the cap (the long
// items at the head of a launch) loads its ids batch by batch.
constexpr int kItemsColumnsIdsCap = 1024;
// IDS16 (DESIGN.md §4.1 "Column halves", slice-local ids): the launch's slots
// hold 16-bit ids local to its source block, `ids` is the plan's uint16 array
// and `ufeat` / `table_bytes` are the block's first row and its bytes (the
// launcher's: the block is shorter than 4 GiB - 1 KiB, the table may be
// longer), so the offsets are block-relative. Lane l still reads slot l of
// its load, a ushort in place of a dword: the same lanes, slots and adds.
// kIds16Aux: the cache policy of those loads (0 default, 2 non-temporal as
// load_row's; both measured, profiles/r32/ids16).
#ifndef DGLHIP_IDS16_AUX
#define DGLHIP_IDS16_AUX 0
#endif
constexpr int kIds16Aux = DGLHIP_IDS16_AUX;

template <int DEPTH, bool ACCUM, bool IDS16>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void
gspmm_items_columns_kernel(
    int64_t num_items, int64_t ldu, uint32_t table_bytes, uint32_t out_bytes,
    const void* __restrict__ ids, const float* __restrict__ ufeat,
    float* __restrict__ out, const int32_t* __restrict__ item_rows,
    const int64_t* __restrict__ item_ptr) {
  static_assert(DEPTH >= 1 && DEPTH <= 16, "a batch's ids are one 16-lane row");
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  typedef std::conditional_t<IDS16, uint16_t, int32_t> id_t;
  const id_t* __restrict__ indices = static_cast<const id_t*>(ids);
  constexpr uint32_t kOff = 0xfffffc00u;  // + any lane offset: past every gated table
  const int lane = threadIdx.x & 63;
  const int q = lane >> 4, ql = lane & 15;
  const int64_t bl = block_linear();
  const int half = static_cast<int>(bl % 8) & 1;
  const int gw = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int64_t wave = (bl >> 1) * (blockDim.x >> 6) + gw;
  const int64_t i0 = wave * 4;
  if (i0 >= num_items) return;
  // quarter t: slots [p[t], p[t + 1]) into row r[t]
  int64_t p[5];
  int64_t r[4];
  if (i0 + 4 <= num_items) {  // uniform: every wave but, at most, the launch's last
    // the nine records in one scalar round trip: wide loads (the arrays are
    // only element-aligned) with nothing between them to wait for
    typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
    typedef int64_t i64x4 __attribute__((ext_vector_type(4)));
    typedef i32x4 i32x4_a4 __attribute__((aligned(4)));
    typedef i64x4 i64x4_a8 __attribute__((aligned(8)));
    const i32x4 rr = *reinterpret_cast<const i32x4_a4*>(item_rows + i0);
    const i64x4 pp = *reinterpret_cast<const i64x4_a8*>(item_ptr + i0);
    p[4] = item_ptr[i0 + 4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      p[t] = pp[t];
      r[t] = rr[t];
    }
  } else {
    // the last wave: none past the last item (a dead quarter has no slots and
    // the last item's row)
#pragma unroll
    for (int t = 0; t < 5; ++t) p[t] = item_ptr[i0 + t < num_items ? i0 + t : num_items];
#pragma unroll
    for (int t = 0; t < 4; ++t) r[t] = item_rows[i0 + t < num_items ? i0 + t : num_items - 1];
  }
  int n[4], rel[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    n[t] = static_cast<int>(p[t + 1] - p[t]);
    rel[t] = static_cast<int>(p[t] - p[0]);
  }
  const int nmin = min(min(n[0], n[1]), min(n[2], n[3]));
  const int nmax = max(max(n[0], n[1]), max(n[2], n[3]));
  const int my_n = q == 0 ? n[0] : (q == 1 ? n[1] : (q == 2 ? n[2] : n[3]));
  const int my_rel = q == 0 ? rel[0] : (q == 1 ? rel[1] : (q == 2 ? rel[2] : rel[3]));
  const uint32_t ld4 = static_cast<uint32_t>(ldu) * 4u;
  const uint32_t lane_off = static_cast<uint32_t>(half) * 256u + static_cast<uint32_t>(ql) * 16u;
  const __amdgpu_buffer_rsrc_t table = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(ufeat), 0, static_cast<int>(table_bytes), 0x00020000);
  // the wave's slots behind a descriptor: a 32-bit offset per id load, and a
  // load past the wave's last slot is answered without a fetch
  const int64_t total = p[4] - p[0];
  const __amdgpu_buffer_rsrc_t slots = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<id_t*>(indices + p[0]), 0,
      static_cast<int>(min(total * int64_t(sizeof(id_t)), int64_t(0x7fffffff))), 0x00020000);
  // the id of the wave's slot s (IDS16: zero-extended)
  auto load_slot = [&](uint32_t s) -> uint32_t {
    if constexpr (IDS16)
      return static_cast<uint16_t>(
          __builtin_amdgcn_raw_buffer_load_b16(slots, s * 2u, 0, kIds16Aux));
    else
      return __builtin_amdgcn_raw_buffer_load_b32(slots, s * 4u, 0, 0);
  };
  // all of out behind one (the gate: shorter than 4 GiB): lane ln's 16 bytes
  // of its quarter's row
  const __amdgpu_buffer_rsrc_t rows = __builtin_amdgcn_make_buffer_rsrc(
      out, 0, static_cast<int>(out_bytes), 0x00020000);
  auto row_offset = [&](int ln) -> uint32_t {
    const int t = ln >> 4;
    const int64_t row = t == 0 ? r[0] : (t == 1 ? r[1] : (t == 2 ? r[2] : r[3]));
    return static_cast<uint32_t>(row) * 512u + static_cast<uint32_t>(half) * 256u +
           static_cast<uint32_t>(ln & 15) * 16u;
  };

  // the running row, non-temporal (RP 2 of load_out). A dead quarter reads the
  // last item's row and stores nothing.
  auto load_row = [&]() -> f32x4 {
    const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(rows, row_offset(lane), 0, 2);
    return *reinterpret_cast<const f32x4*>(&w);
  };
  // the wave's region of LDS: the byte offsets of its slots' rows
  __shared__ uint32_t ids_lds[4][kItemsColumnsIdsCap];
  uint32_t* const wids = ids_lds[gw];

  f32x4 acc = Vec<4>::zero();
  // The wave's batches. PRELOADED: the wave's offsets go to LDS first and the
  // batches read them there; otherwise a batch's ids come from memory.
  auto batches = [&](auto preloaded) {
    constexpr bool PRELOADED = decltype(preloaded)::value;
    // this lane's share of the batch at slot k: the id of slot k + ql of its
    // quarter's item (PRELOADED: the offset already), then the byte offset of
    // that row (past the item's end: past the table). The load stays inside
    // the wave's slots (an ended item re-reads its last id, an empty one a
    // neighbour's), so it needs no predicate, also for a batch that does not
    // come.
    auto load_ids = [&](int k) -> uint32_t {
      const int s = max(min(k + ql, my_n - 1) + my_rel, 0);
      if constexpr (PRELOADED) return wids[s];
      else
        return load_slot(static_cast<uint32_t>(s));
    };
    auto offsets = [&](uint32_t id, int k) -> uint32_t {
      return k + ql < my_n ? (PRELOADED ? id : id * ld4) : kOff;
    };
    // the first ids leave ahead of the running row, which comes from the
    // fabric and is not needed before the first add: the gathers wait for the
    // ids alone. (Vector loads return in order. The barriers keep the
    // compiler's scheduler from swapping the two; the empty asm is the first
    // use of the ids, where the wait goes.)
    uint32_t raw;
    if constexpr (PRELOADED) {
      // 256 slots per group of loads: lane l reads slots c + 64u + l, a load
      // and its write behind a uniform branch, the lanes past the last slot
      // switched off by the descriptor (load) and the predicate (write). A
      // wave of more than 256 slots (one in fifty) goes round again.
      const int T = static_cast<int>(total);
      uint32_t g[4];
      auto load_group = [&](int c) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (u == 0 || c + 64 * u < T)
            g[u] = load_slot(static_cast<uint32_t>(c + 64 * u + lane));
        }
      };
      auto write_group = [&](int c) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (u == 0 || c + 64 * u < T) {
            const int s = c + 64 * u + lane;
            if (s < T) wids[s] = g[u] * ld4;
          }
        }
      };
      load_group(0);
      __builtin_amdgcn_sched_barrier(0);
      if (ACCUM) acc = load_row();
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("" : "+v"(g[0]));
      write_group(0);
#pragma unroll 1
      for (int c = 256; c < T; c += 256) {
        load_group(c);
        write_group(c);
        // (vmcnt(0), as the writes have waited: said for the compiler, which
        // cannot count loads behind uniform branches and would wait for the
        // running row ahead of the first LDS read)
        __builtin_amdgcn_s_waitcnt(0x0f70);
      }
      // the writes ahead of the reads, also for the compiler
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      raw = load_ids(0);
    } else {
      raw = load_ids(0);
      __builtin_amdgcn_sched_barrier(0);
      if (ACCUM) acc = load_row();
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("" : "+v"(raw));
    }
    uint32_t ids = offsets(raw, 0);
    int k = 0;
    // every item has DEPTH slots left: every lane gathers, no predicate
#pragma unroll 1
    for (; k + DEPTH <= nmin; k += DEPTH) {
      u32x4 v[DEPTH];
#pragma unroll
      for (int j = 0; j < DEPTH; ++j)
        v[j] = __builtin_amdgcn_raw_buffer_load_b128(table, row_broadcast(ids, j) + lane_off, 0,
                                                     0);
      // the next batch's ids behind the gathers, not looked at before the
      // batch's last add: each add waits for its own gather only, and the id
      // round trip (a first touch, from the fabric; PRELOADED: an LDS read)
      // runs beside the chain
      raw = load_ids(k + DEPTH);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < DEPTH; ++j) acc += *reinterpret_cast<const f32x4*>(&v[j]);
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("" : "+v"(raw));
      ids = offsets(raw, k + DEPTH);
    }
    // the rest as predicated batches, every gather of a batch in flight
    // together; a lane whose item has no slot k + j gathers past the table and
    // does not add the value (not even a zero: -0.0 + 0.0 is +0.0)
#pragma unroll 1
    for (; k < nmax; k += DEPTH) {
      const int rb = nmax - k;
      u32x4 v[DEPTH];
#pragma unroll
      for (int j = 0; j < DEPTH; ++j) {
        if (j < rb)  // uniform
          v[j] = __builtin_amdgcn_raw_buffer_load_b128(table, row_broadcast(ids, j) + lane_off,
                                                       0, 0);
      }
      raw = load_ids(k + DEPTH);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < DEPTH; ++j) {
        if (j < rb) {
          const f32x4 sum = acc + *reinterpret_cast<const f32x4*>(&v[j]);
          acc = k + j < my_n ? sum : acc;
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      // PRELOADED: no vector load closes the batch, and the compiler cannot
      // count gathers behind uniform branches: told here that all have landed
      // (vmcnt(0), which the adds have waited for), it does not wait for the
      // whole batch again ahead of each gather of the next one
      if constexpr (PRELOADED) __builtin_amdgcn_s_waitcnt(0x0f70);
      asm volatile("" : "+v"(raw));
      ids = offsets(raw, k + DEPTH);
    }
  };
  if (nmax > 0) {
    // uniform: all but the long items at the head of a launch
    if (total <= kItemsColumnsIdsCap) batches(std::true_type{});
    else batches(std::false_type{});
  } else if (ACCUM) {
    acc = load_row();
  }
  // one store for the wave's four rows (sc1: the lines leave the XCD's L2, RP
  // 2 / 4 of store_out), the quarters past the last item switched off. The
  // lane's place is worked out again from its id in the wave: held across the
  // batches it would be the 65th register.
  const int ln = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  if (i0 + (ln >> 4) < num_items)
    __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4*>(&acc), rows,
                                           row_offset(ln), 0, 16);
}

// One launch of the blocked schedule's items. The first nine fields are all
// the gate looks at (dglhip_gspmm_items_kernel takes them in this order).
struct ItemsLaunch {
  int msg;
  int64_t F;
  int64_t ldu;         // ufeat row stride in elements (0: F)
  int64_t urows;       // rows of ufeat (0: not known)
  int64_t orows;       // rows of out (0: not known)
  int items_per_wave;  // 2: gspmm_items_pair_kernel where it applies
  int column_parts;    // 2: gspmm_items_columns_kernel where it applies
  const float* ufeat;
  float* out;
  int64_t num_items;
  const int32_t* item_rows;
  const int64_t* item_ptr;
  const int32_t* indices;
  bool accumulate;
  // 16-bit ids local to the launch's source block (nullptr: indices): rows
  // [col_lo, col_lo + block_rows) of ufeat, slot s gathering row col_lo + ids16[s]
  const uint16_t* ids16 = nullptr;
  int64_t col_lo = 0;
  int64_t block_rows = 0;
};

// Whether a copy_u launch of the blocked schedule's items takes the two-
// items-per-wave kernel: fp32 rows of 128 floats, 16-byte lanes (the table,
// its row stride and out aligned to them) and 32-bit gather offsets (the
// table shorter than 4 GiB, which needs its row count).
static inline bool items_pair_applies(const ItemsLaunch& a) {
  const int64_t ldu = a.ldu ? a.ldu : a.F;
  return a.items_per_wave == 2 && a.F == 128 && a.urows > 0 && ldu % 4 == 0 &&
         reinterpret_cast<uintptr_t>(a.ufeat) % 16 == 0 &&
         reinterpret_cast<uintptr_t>(a.out) % 16 == 0 &&
         a.urows * ldu * int64_t(sizeof(float)) < (int64_t(1) << 32);
}

// Whether it takes the column-half kernel instead: the pair kernel's gate,
// and a table that ends 1 KiB below 4 GiB (a switched-off lane's offset plus
// its column offset must neither wrap nor fall inside the table), and 32-bit
// offsets into out for the wave's one store: out shorter than 4 GiB, which
// needs its row count.
static inline bool items_columns_applies(const ItemsLaunch& a) {
  const int64_t ldu = a.ldu ? a.ldu : a.F;
  return a.column_parts == 2 && items_pair_applies(a) &&
         a.urows * ldu * int64_t(sizeof(float)) <= int64_t(0xfffffc00u) && a.orows > 0 &&
         a.orows * a.F * int64_t(sizeof(float)) < (int64_t(1) << 32);
}

// Whether a launch with 16-bit block-local ids takes the column-half kernel:
// its gate with the block's bytes in place of the whole table's (the
// descriptor covers the block alone, so a table past 4 GiB qualifies block by
// block), ids that fit 16 bits, and the block inside the table.
static inline bool items_columns_ids16_applies(const ItemsLaunch& a) {
  const int64_t ldu = a.ldu ? a.ldu : a.F;
  return a.ids16 != nullptr && a.msg == DGLHIP_MSG_COPY_U && a.items_per_wave == 2 &&
         a.column_parts == 2 && a.F == 128 && ldu % 4 == 0 &&
         reinterpret_cast<uintptr_t>(a.ufeat) % 16 == 0 &&
         reinterpret_cast<uintptr_t>(a.out) % 16 == 0 && a.col_lo >= 0 && a.block_rows > 0 &&
         a.block_rows <= 65536 && a.col_lo + a.block_rows <= a.urows &&
         a.block_rows * ldu * int64_t(sizeof(float)) <= int64_t(0xfffffc00u) && a.orows > 0 &&
         a.orows * a.F * int64_t(sizeof(float)) < (int64_t(1) << 32);
}

// The kernel of a launch: 0 one item per wave (the generic sum kernel), 1
// gspmm_items_pair_kernel, 2 gspmm_items_columns_kernel. Looks at the
// numbers and the two addresses only. The message and the two predicates are
// the whole condition, i.e. the launches that the generic dispatch would give
// launch_sum<2, 64, COPY_U, EM_SCALAR, MEAN = false> with item rows and plain
// stores: the kernels add fp32 source rows, so the message is the fp32 copy_u
// (the bf16 one is a message of its own); copy_u has no edge operand (elen 1,
// the scalar layout); F = 128 with ufeat and out 16-byte aligned is pick_vec
// 2 and pick_group 64; the items entries ask for a sum, never a mean, and
// never for non-temporal stores; item_rows and item_ptr are given (checked
// before the gate is asked).
static int items_kernel(const ItemsLaunch& a) {
  if (a.msg != DGLHIP_MSG_COPY_U || !items_pair_applies(a)) return 0;
  return items_columns_applies(a) ? 2 : 1;
}

static inline void launch_items_columns(const ItemsLaunch& a, hipStream_t stream) {
  // 12 gathers in flight per lane: the most that keep 64 VGPRs, so 8 waves per
  // SIMD (8 / 10 / 12 / 14 / 16 measured: DESIGN.md §4.1 "Column halves")
  constexpr int DEPTH = 12;
  // 16 items (4 waves of 4) per pair of blocks, one block per column half
  const int64_t blocks = 2 * ((a.num_items + 15) / 16);
  DGLHIP_CHECK(blocks <= 0x7fffffff, "grid too large: " << blocks);
  const int64_t ldu = a.ldu ? a.ldu : a.F;
  // 16-bit ids: the table the kernel sees is the launch's source block
  const bool ids16 = a.ids16 != nullptr;
  auto kernel = ids16 ? (a.accumulate ? gspmm_items_columns_kernel<DEPTH, true, true>
                                      : gspmm_items_columns_kernel<DEPTH, false, true>)
                      : (a.accumulate ? gspmm_items_columns_kernel<DEPTH, true, false>
                                      : gspmm_items_columns_kernel<DEPTH, false, false>);
  const int64_t rows = ids16 ? a.block_rows : a.urows;
  const float* table = ids16 ? a.ufeat + a.col_lo * ldu : a.ufeat;
  const void* ids = ids16 ? static_cast<const void*>(a.ids16) : a.indices;
  timed_launch(stream, [&] {
    hipLaunchKernelGGL(kernel, grid_1d(blocks), dim3(256), 0, stream, a.num_items, ldu,
                       static_cast<uint32_t>(rows * ldu * int64_t(sizeof(float))),
                       static_cast<uint32_t>(a.orows * a.F * int64_t(sizeof(float))), ids, table,
                       a.out, a.item_rows, a.item_ptr);
  });
}

static inline void launch_items_pair(const ItemsLaunch& a, hipStream_t stream) {
  // 10 pairs of rows in flight per wave: the most that keep 64 VGPRs, so 8
  // waves per SIMD (8 / 10 / 12 / 16 measured: DESIGN.md §4.1 "Two items per wave")
  constexpr int DEPTH = 10;
  const int64_t blocks = (a.num_items + 7) / 8;  // 4 waves of 2 items
  DGLHIP_CHECK(blocks <= 0x7fffffff, "grid too large: " << blocks);
  const int64_t ldu = a.ldu ? a.ldu : a.F;
  auto kernel = a.accumulate ? gspmm_items_pair_kernel<DEPTH, true>
                             : gspmm_items_pair_kernel<DEPTH, false>;
  timed_launch(stream, [&] {
    hipLaunchKernelGGL(kernel, grid_1d(blocks), dim3(256), 0, stream, a.num_items, ldu,
                       static_cast<uint32_t>(a.urows * ldu * int64_t(sizeof(float))), a.indices,
                       a.ufeat, a.out, a.item_rows, a.item_ptr);
  });
}

void gspmm_items_columns(int msg_op, int64_t num_items, int64_t feat_len, const int32_t* item_rows,
                         const int64_t* item_ptr, int accumulate, const int32_t* indices,
                         const int64_t* eid, const float* ufeat, int64_t ufeat_ld,
                         int64_t ufeat_rows, int items_per_wave, int column_parts,
                         const float* efeat, int64_t efeat_len, float* out, int64_t out_rows,
                         hipStream_t stream) {
  DGLHIP_CHECK(msg_op >= 0 && msg_op <= 3, "unknown msg op " << msg_op);
  DGLHIP_CHECK(num_items >= 0 && feat_len >= 0 && ufeat_rows >= 0 && out_rows >= 0,
               "negative size");
  DGLHIP_CHECK(items_per_wave == 1 || items_per_wave == 2,
               "items_per_wave " << items_per_wave << ": 1 or 2");
  DGLHIP_CHECK(column_parts == 1 || column_parts == 2,
               "column_parts " << column_parts << ": 1 or 2");
  if (num_items == 0 || feat_len == 0) return;
  DGLHIP_CHECK(item_rows && item_ptr && indices && out, "null items/indices/out");
  const int64_t elen = check_operands(msg_op, feat_len, ufeat, efeat, efeat_len);
  check_ufeat_ld(ufeat_ld, feat_len);
  const ItemsLaunch a{msg_op, feat_len, ufeat_ld, ufeat_rows, out_rows, items_per_wave,
                      column_parts, ufeat, out, num_items, item_rows, item_ptr, indices,
                      accumulate != 0};
  switch (items_kernel(a)) {
    case 2: launch_items_columns(a, stream); break;
    case 1: launch_items_pair(a, stream); break;
    default:
      gspmm_items_one(msg_op, num_items, feat_len, elen, item_rows, item_ptr, accumulate != 0,
                      indices, eid, ufeat, ufeat_ld, efeat, out, stream);
  }
}

bool gspmm_items_columns_ids16(int64_t num_items, const int32_t* item_rows,
                               const int64_t* item_ptr, int accumulate, const uint16_t* ids16,
                               int64_t col_lo, int64_t block_rows, const float* ufeat,
                               int64_t ufeat_ld, int64_t ufeat_rows, float* out, int64_t out_rows,
                               hipStream_t stream) {
  DGLHIP_CHECK(num_items >= 0 && ufeat_rows >= 0 && out_rows >= 0, "negative size");
  if (num_items == 0) return true;
  DGLHIP_CHECK(item_rows && item_ptr && ids16 && ufeat && out, "null items/ids/ufeat/out");
  check_ufeat_ld(ufeat_ld, 128);
  ItemsLaunch a{DGLHIP_MSG_COPY_U, 128, ufeat_ld, ufeat_rows, out_rows, 2, 2, ufeat, out,
                num_items, item_rows, item_ptr, nullptr, accumulate != 0};
  a.ids16 = ids16;
  a.col_lo = col_lo;
  a.block_rows = block_rows;
  if (!items_columns_ids16_applies(a)) return false;
  launch_items_columns(a, stream);
  return true;
}

}  // namespace dglhip

using namespace dglhip;

extern "C" {

int dglhip_gspmm_items_kernel(int msg_op, int64_t feat_len, int64_t ufeat_ld, int64_t ufeat_rows,
                              int64_t out_rows, int items_per_wave, int column_parts,
                              const float* ufeat, const float* out, int* kernel) {
  API_BEGIN();
  DGLHIP_CHECK(kernel != nullptr, "null pointer argument");
  *kernel = items_kernel(ItemsLaunch{msg_op, feat_len, ufeat_ld, ufeat_rows, out_rows,
                                     items_per_wave, column_parts, ufeat,
                                     const_cast<float*>(out)});
  API_END();
}

int dglhip_gspmm_items_columns_ids_cap(void) { return kItemsColumnsIdsCap; }

int dglhip_gspmm_items_columns_device(int msg_op, int64_t num_items, int64_t feat_len,
                                      const int32_t* item_rows, const int64_t* item_ptr,
                                      int accumulate, const int32_t* indices, const int64_t* eid,
                                      const float* ufeat, int64_t ufeat_ld, int64_t ufeat_rows,
                                      int items_per_wave, int column_parts, const float* efeat,
                                      int64_t efeat_len, float* out, void* stream_) {
  API_BEGIN();
  // the rows of out are not among the arguments: column_parts 2 runs the pair
  // kernel here (the same bits); the plan calls gspmm_items_columns itself
  gspmm_items_columns(msg_op, num_items, feat_len, item_rows, item_ptr, accumulate, indices, eid,
                      ufeat, ufeat_ld, ufeat_rows, items_per_wave, column_parts, efeat, efeat_len,
                      out, 0, static_cast<hipStream_t>(stream_));
  API_END();
}

int dglhip_gspmm_items_ids16_device(int64_t num_items, const int32_t* item_rows,
                                    const int64_t* item_ptr, int accumulate,
                                    const uint16_t* ids16, int64_t col_lo, int64_t block_rows,
                                    const float* ufeat, int64_t ufeat_ld, int64_t ufeat_rows,
                                    float* out, int64_t out_rows, void* stream_) {
  API_BEGIN();
  // this entry is the 16-bit kernel or nothing: no other kernel reads these ids
  DGLHIP_CHECK(gspmm_items_columns_ids16(num_items, item_rows, item_ptr, accumulate, ids16, col_lo,
                                         block_rows, ufeat, ufeat_ld, ufeat_rows, out, out_rows,
                                         static_cast<hipStream_t>(stream_)),
               "16-bit ids: rows [" << col_lo << ", " << col_lo + block_rows << ") of "
                                    << ufeat_rows << " into " << out_rows
                                    << " rows do not take the column-half kernel");
  API_END();
}

int dglhip_gspmm_items_table_device(int msg_op, int64_t num_items, int64_t feat_len,
                                    const int32_t* item_rows, const int64_t* item_ptr,
                                    int accumulate, const int32_t* indices, const int64_t* eid,
                                    const float* ufeat, int64_t ufeat_ld, int64_t ufeat_rows,
                                    int items_per_wave, const float* efeat, int64_t efeat_len,
                                    float* out, void* stream_) {
  return dglhip_gspmm_items_columns_device(msg_op, num_items, feat_len, item_rows, item_ptr,
                                           accumulate, indices, eid, ufeat, ufeat_ld, ufeat_rows,
                                           items_per_wave, 1, efeat, efeat_len, out, stream_);
}

int dglhip_gspmm_items_device(int msg_op, int64_t num_items, int64_t feat_len,
                              const int32_t* item_rows, const int64_t* item_ptr, int accumulate,
                              const int32_t* indices, const int64_t* eid, const float* ufeat,
                              int64_t ufeat_ld, const float* efeat, int64_t efeat_len,
                              float* out, void* stream_) {
  return dglhip_gspmm_items_table_device(msg_op, num_items, feat_len, item_rows, item_ptr,
                                         accumulate, indices, eid, ufeat, ufeat_ld, 0, 1, efeat,
                                         efeat_len, out, stream_);
}

}  // extern "C"

