// The neighbour-sampling rules, defined once for the device kernels
// (neighbor_sample.hip) and the host twin (neighbor_sample_host.cc).
//
// Uniform. Slot p of the row of vertex v gets the key
//   key(seed, v, p) = mix(mix(mix(seed) ^ v) ^ p)
// with mix the splitmix64 finaliser. A row of d slots at fan-out k keeps every
// slot when d <= k, else the k positions with the smallest (key, p) pairs (a
// tie on the key goes to the smaller p), emitted in ascending p. The keys are
// independent of each other and of any state, so the k smallest are a uniform
// k-subset and a wave, a host loop and a numpy restatement pick the same one.
//
// Weighted (node_weight, float32 per node): the Efraimidis-Spirakis
// exponential race. With h the uniform key of the slot and w the weight of
// the slot's neighbour,
//   m = (h >> 11) + 1          an integer in [1, 2^53]; u = m 2^-53 in (0, 1]
//   E = sample_neglog(m)       ~ -ln u, a double >= 0
//   key = bits(E / double(w))  when w is positive, normal and finite,
//         0x7FF0000000000000   for any other w (zero, denormal, negative,
//                              infinity, NaN) and for a neighbour outside the
//                              graph: the slot is weightless.
// Non-negative doubles order like their bit patterns, so the selection above
// runs on these keys unchanged: the k smallest E / w are k successive draws
// proportional to w without replacement, and weightless slots fill a sample
// only when fewer than k slots carry weight, first positions first.
//
// sample_neglog uses integer operations and IEEE double +, -, *, / only, each
// rounded on its own (no contraction into FMAs, no library logarithm), so the
// device, host C++ and numpy produce the same bits:
//   e = floor(log2 m); f = m 2^-e in [1, 2); if f > SQRT2: f /= 2, e += 1
//   s = (f - 1) / (f + 1); t = s s                        (|s| <= 0.1716)
//   ln f = s (2 + t (2/3 + t (2/5 + ... + t 2/19)))       ten terms, Horner
//   E = (53 - e) LN2 - ln f, and 0 where that is negative.
// The first dropped term is below 5e-18.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DGLHIP_SAMPLE_FN __host__ __device__ inline
#else
#define DGLHIP_SAMPLE_FN inline
#endif

// Every double operation of a function so marked is rounded on its own.
#if defined(__clang__)
#define DGLHIP_SAMPLE_STRICT_FN DGLHIP_SAMPLE_FN
#define DGLHIP_SAMPLE_STRICT_BODY _Pragma("clang fp contract(off)")
#else
#define DGLHIP_SAMPLE_STRICT_FN __attribute__((optimize("fp-contract=off"))) DGLHIP_SAMPLE_FN
#define DGLHIP_SAMPLE_STRICT_BODY
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

// The key of a weightless slot: above every weighted one.
constexpr uint64_t kSampleWeightless = 0x7FF0000000000000ull;

DGLHIP_SAMPLE_FN double sample_bits_to_double(uint64_t bits) {
  double x;
  __builtin_memcpy(&x, &bits, sizeof(x));
  return x;
}

// -ln(m 2^-53) for m in [1, 2^53] (0 is taken as 1; of a larger m the top 53
// bits are used). sample_neglog(2^53) == 0.
DGLHIP_SAMPLE_STRICT_FN double sample_neglog(uint64_t m) {
  DGLHIP_SAMPLE_STRICT_BODY
  if (m == 0) m = 1;
  int e = 63 - __builtin_clzll(m);
  const uint64_t frac = (e <= 52 ? m << (52 - e) : m >> (e - 52)) & 0x000FFFFFFFFFFFFFull;
  double f = sample_bits_to_double(0x3FF0000000000000ull | frac);  // m 2^-e, exact
  if (f > 1.4142135623730951) {
    f = f * 0.5;
    e += 1;
  }
  const double s = (f - 1.0) / (f + 1.0);
  const double t = s * s;
  double r = 0.10526315789473684;       // 2/19
  r = 0.11764705882352941 + t * r;      // 2/17
  r = 0.13333333333333333 + t * r;      // 2/15
  r = 0.15384615384615385 + t * r;      // 2/13
  r = 0.18181818181818182 + t * r;      // 2/11
  r = 0.2222222222222222 + t * r;       // 2/9
  r = 0.2857142857142857 + t * r;       // 2/7
  r = 0.4 + t * r;                      // 2/5
  r = 0.6666666666666666 + t * r;       // 2/3
  r = 2.0 + t * r;
  const double lnf = s * r;
  const double E = static_cast<double>(53 - e) * 0.6931471805599453 - lnf;
  return E < 0.0 ? 0.0 : E;
}

// The weighted key of a slot whose uniform key is h and whose neighbour's
// weight has the bit pattern wbits.
DGLHIP_SAMPLE_STRICT_FN uint64_t sample_weighted_slot_key(uint64_t h, uint32_t wbits) {
  DGLHIP_SAMPLE_STRICT_BODY
  const uint32_t expo = (wbits >> 23) & 0xFFu;
  if ((wbits >> 31) != 0 || expo == 0 || expo == 0xFFu) return kSampleWeightless;
  float w;
  __builtin_memcpy(&w, &wbits, sizeof(w));
  const double q = sample_neglog((h >> 11) + 1) / static_cast<double>(w);
  uint64_t bits;
  __builtin_memcpy(&bits, &q, sizeof(bits));
  return bits;
}

DGLHIP_SAMPLE_FN uint64_t sample_weighted_key(uint64_t seed, int64_t v, int64_t p, float w) {
  uint32_t wbits;
  __builtin_memcpy(&wbits, &w, sizeof(wbits));
  return sample_weighted_slot_key(sample_key(seed, v, p), wbits);
}

}  // namespace dglhip
