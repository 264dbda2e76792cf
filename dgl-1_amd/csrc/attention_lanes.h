// Device helpers of the fused attention kernels (dot_attention.hip,
// gatv2_attention.hip, through attention_walk.h): a lane's vector accesses, the xor butterfly that sums
// across the lanes of a head, and the hand-out of a row's column ids in
// batches. Both units compute their per-edge sums with these, in a fixed
// order: the same bits in every kernel that recomputes a score.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dglhip {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int V>
__device__ __forceinline__ void load_vec(const float* p, float (&v)[V]) {
  if constexpr (V == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  } else if constexpr (V == 2) {
    const f32x2 t = *reinterpret_cast<const f32x2*>(p);
    v[0] = t[0]; v[1] = t[1];
  } else {
    v[0] = *p;
  }
}

template <int V>
__device__ __forceinline__ void store_vec(float* p, const float (&v)[V]) {
  if constexpr (V == 4) {
    f32x4 t;
    t[0] = v[0]; t[1] = v[1]; t[2] = v[2]; t[3] = v[3];
    *reinterpret_cast<f32x4*>(p) = t;
  } else if constexpr (V == 2) {
    f32x2 t;
    t[0] = v[0]; t[1] = v[1];
    *reinterpret_cast<f32x2*>(p) = t;
  } else {
    *p = v[0];
  }
}

// torch's max: a NaN on either side wins (fmaxf would drop it)
__device__ __forceinline__ float nanmax(float a, float b) { return (a > b || a != a) ? a : b; }

// a value every lane of the wave holds, told to the compiler
__device__ __forceinline__ int64_t uniform64(int64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(uint64_t(v) >> 32));
  return static_cast<int64_t>((uint64_t(hi) << 32) | lo);
}

template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}

// N sums across the 1 << sh lanes of a head, stage by stage: DPP at strides
// 1, 2 (quad permutes), 4, 8 (the mirrors of 8 and 16 lanes: after the earlier
// stages a mirror's partner holds what the xor partner holds), __shfl_xor at
// 16 and 32. Both partners of a stage add the same two numbers, so every lane
// of a head ends with the same bits. Every lane of the wave must call it.
template <int N>
__device__ __forceinline__ void head_sum(float (&x)[N], int sh) {
  if (sh >= 1) {
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = x[i] + dpp<0xB1>(x[i]);  // quad_perm [1,0,3,2]
  }
  if (sh >= 2) {
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = x[i] + dpp<0x4E>(x[i]);  // quad_perm [2,3,0,1]
  }
  if (sh >= 3) {
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = x[i] + dpp<0x141>(x[i]);  // row_half_mirror
  }
  if (sh >= 4) {
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = x[i] + dpp<0x140>(x[i]);  // row_mirror
  }
  if (sh >= 5) {
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = x[i] + __shfl_xor(x[i], 16, 64);
  }
  if (sh >= 6) {
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = x[i] + __shfl_xor(x[i], 32, 64);
  }
}

// The slots [k0, k1) (the same in every lane) in batches: the wave takes up
// to 64 column ids in one coalesced load and hands them out lane to lane;
// body(u, n) gets BATCH column ids, clamped to the C columns, of which the
// first n (>= 1; n > BATCH means all) are the batch's slots and the rest
// repeat its last one, so every gather has an address.
template <int BATCH, typename Body>
__device__ __forceinline__ void batch_ids(const int32_t* indices, int64_t C, int64_t k0,
                                          int64_t k1, int lane, Body&& body) {
  for (int64_t base = k0; base < k1; base += 64) {
    const int n = k1 - base < 64 ? static_cast<int>(k1 - base) : 64;
    int mine = 0;
    if (lane < n) {
      mine = indices[base + lane];
      mine = mine < 0 ? 0 : (mine > C - 1 ? static_cast<int>(C - 1) : mine);
    }
    for (int j0 = 0; j0 < n; j0 += BATCH) {
      int u[BATCH];
#pragma unroll
      for (int i = 0; i < BATCH; ++i) u[i] = __shfl(mine, j0 + i < n ? j0 + i : n - 1, 64);
      body(u, n - j0);
    }
  }
}

}  // namespace dglhip
