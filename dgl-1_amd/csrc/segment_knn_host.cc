// Segment k-nearest neighbours on the host: segment_knn.hip's contract by
// brute force, a partial sort of the packed words bits(d) << 32 | row within
// the segment per query on the thread pool. Float32 by the same formula
// (norm + norm - 2 dot, values not above zero set to +0.0, d(i, i) = +0.0, a
// NaN keyed after +inf). The sums are plain fma chains, the device's are the
// MFMA's: each side returns the exact top-k under its own distances, and the
// same answer wherever the arithmetic is exact.
#include "../../include/dgl_hip.h"
#include "common.h"

#include <cmath>
#include <cstring>

namespace dglhip {

namespace {

inline float dot(const float* p, const float* q, int64_t D) {
  float s = 0.0f;
  for (int64_t c = 0; c < D; ++c) s = std::fmaf(p[c], q[c], s);
  return s;
}

}  // namespace

}  // namespace dglhip

using namespace dglhip;

extern "C" {

int dglhip_segment_knn_host(int64_t num_segments, int64_t num_rows, int64_t dim, int64_t k,
                            int exclude_self, const int64_t* offsets, const float* x,
                            int64_t ldx, int64_t* nbr, float* dist, int num_threads) {
  API_BEGIN();
  const int64_t B = num_segments, N = num_rows, D = dim;
  DGLHIP_CHECK(B >= 0 && N >= 0 && D >= 0, "negative size");
  DGLHIP_CHECK(k >= 1 && k <= DGLHIP_KNN_MAX_K,
               "k = " << k << " outside [1, DGLHIP_KNN_MAX_K = " << DGLHIP_KNN_MAX_K << "]");
  DGLHIP_CHECK(D >= 1 && D <= DGLHIP_KNN_MAX_DIM,
               "D = " << D << " outside [1, DGLHIP_KNN_MAX_DIM = " << DGLHIP_KNN_MAX_DIM << "]");
  DGLHIP_CHECK(N < (int64_t(1) << 31), "num_rows must be below 2^31");
  DGLHIP_CHECK(offsets != nullptr, "offsets is null");
  DGLHIP_CHECK(offsets[0] == 0, "offsets must start at 0, got " << offsets[0]);
  for (int64_t s = 0; s < B; ++s)
    DGLHIP_CHECK(offsets[s + 1] >= offsets[s], "offsets decrease at segment " << s);
  DGLHIP_CHECK(offsets[B] == N, "offsets end at " << offsets[B] << ", expected the " << N
                                                  << " rows");
  if (B == 0 || N == 0) return 0;
  DGLHIP_CHECK(x && nbr && dist, "null pointer argument");
  DGLHIP_CHECK(ldx >= D, "row stride below the row width");
  const int nt = num_threads > 0 ? num_threads : default_num_threads();
  std::vector<float> norms(N);
  parallel_for(N, nt, [&](int64_t i0, int64_t i1, int) {
    for (int64_t i = i0; i < i1; ++i) norms[i] = dot(x + i * ldx, x + i * ldx, D);
  });
  // the segment of every query row, so that the rows (not the segments) are split
  std::vector<int64_t> seg(N);
  for (int64_t s = 0; s < B; ++s) std::fill(seg.begin() + offsets[s], seg.begin() + offsets[s + 1], s);
  const bool skip = exclude_self != 0;
  parallel_for(N, nt, [&](int64_t i0, int64_t i1, int) {
    std::vector<uint64_t> w;
    for (int64_t i = i0; i < i1; ++i) {
      const int64_t beg = offsets[seg[i]], n = offsets[seg[i] + 1] - beg;
      w.clear();
      for (int64_t c = 0; c < n; ++c) {
        const int64_t j = beg + c;
        if (j == i && skip) continue;
        const float v = (norms[i] + norms[j]) - 2.0f * dot(x + i * ldx, x + j * ldx, D);
        const float d = j == i ? 0.0f : (v > 0.0f ? v : (v == v ? 0.0f : v));
        uint32_t bits = 0x7fc00000u;
        if (d == d) std::memcpy(&bits, &d, 4);
        w.push_back((uint64_t(bits) << 32) | static_cast<uint32_t>(c));
      }
      const int64_t m = std::min<int64_t>(k, static_cast<int64_t>(w.size()));
      std::partial_sort(w.begin(), w.begin() + m, w.end());
      for (int64_t j = 0; j < k; ++j) {
        const uint32_t bits = j < m ? static_cast<uint32_t>(w[j] >> 32) : 0x7f800000u;
        nbr[i * k + j] = j < m ? beg + static_cast<int64_t>(static_cast<uint32_t>(w[j])) : -1;
        std::memcpy(dist + i * k + j, &bits, 4);
      }
    }
  }, 16);
  API_END();
}

}  // extern "C"
