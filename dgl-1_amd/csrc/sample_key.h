// The uniform neighbour-sampling rule, defined once for the device kernels
// (neighbor_sample.hip) and the host twin (neighbor_sample_host.cc).
//
// Slot p of the row of vertex v gets the key
//   key(seed, v, p) = mix(mix(mix(seed) ^ v) ^ p)
// with mix the splitmix64 finaliser. A row of d slots at fan-out k keeps every
// slot when d <= k, else the k positions with the smallest (key, p) pairs (a
// tie on the key goes to the smaller p), emitted in ascending p. The keys are
// independent of each other and of any state, so the k smallest are a uniform
// k-subset and a wave, a host loop and a numpy restatement pick the same one.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DGLHIP_SAMPLE_FN __host__ __device__ inline
#else
#define DGLHIP_SAMPLE_FN inline
#endif

namespace dglhip {

// mix(0) == 0xE220A8397B1DCDAF
DGLHIP_SAMPLE_FN uint64_t sample_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// The part of the key shared by the slots of one row.
DGLHIP_SAMPLE_FN uint64_t sample_row_base(uint64_t seed, int64_t v) {
  return sample_mix(sample_mix(seed) ^ static_cast<uint64_t>(v));
}

DGLHIP_SAMPLE_FN uint64_t sample_slot_key(uint64_t row_base, int64_t p) {
  return sample_mix(row_base ^ static_cast<uint64_t>(p));
}

DGLHIP_SAMPLE_FN uint64_t sample_key(uint64_t seed, int64_t v, int64_t p) {
  return sample_slot_key(sample_row_base(seed, v), p);
}

}  // namespace dglhip
