// What the host forms of the attention operators share (dot_attention_host.cc,
// gatv2_attention_host.cc; edge_softmax_host.cc takes nanmax): the CSR check,
// the float32 helpers and the forward's softmax-aggregate pass over a row.
#pragma once

#include "common.h"

#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

namespace dglhip {

inline void check_csr(int64_t R, int64_t C, int64_t nnz, const int64_t* indptr,
                      const int32_t* indices) {
  DGLHIP_CHECK(indptr != nullptr, "indptr is null");
  DGLHIP_CHECK(indptr[0] == 0, "indptr must start at 0, got " << indptr[0]);
  for (int64_t r = 0; r < R; ++r)
    DGLHIP_CHECK(indptr[r + 1] >= indptr[r], "indptr decreases at row " << r);
  DGLHIP_CHECK(indptr[R] == nnz, "indptr ends at " << indptr[R] << ", expected the " << nnz
                                                   << " slots");
  DGLHIP_CHECK(nnz == 0 || indices != nullptr, "indices is null");
  for (int64_t k = 0; k < nnz; ++k)
    DGLHIP_CHECK(indices[k] >= 0 && indices[k] < C, "column " << indices[k] << " of slot " << k
                                                              << " out of range");
}

// torch's max: a NaN on either side wins
inline float nanmax(float a, float b) { return (a > b || a != a) ? a : b; }

inline float dot(const float* x, const float* y, int64_t D) {
  float t = 0.0f;
  for (int64_t d = 0; d < D; ++d) t += x[d] * y[d];
  return t;
}

inline int threads_of(int num_threads) {
  return num_threads > 0 ? num_threads : default_num_threads();
}

// The forward over the rows [r0, r1): per (row, head) the scores
// score(r, h, j) of the slots j, their maximum, then in slot order
// e = exp(s - m), l += e, out += e * val[column of j], and out / l with
// lse = m + log(l); zeros for a row without slots. val is (columns, H, D).
template <typename Score>
void softmax_aggregate_rows(int64_t r0, int64_t r1, int64_t H, int64_t D, const int64_t* indptr,
                            const int32_t* indices, const float* val, float* out, float* lse,
                            Score&& score) {
  const int64_t F = H * D;
  std::vector<float> s;
  for (int64_t r = r0; r < r1; ++r) {
    const int64_t beg = indptr[r], end = indptr[r + 1];
    s.resize(end - beg);
    for (int64_t h = 0; h < H; ++h) {
      float* o = out + r * F + h * D;
      for (int64_t d = 0; d < D; ++d) o[d] = 0.0f;
      if (beg == end) {
        lse[r * H + h] = 0.0f;
        continue;
      }
      float m = -std::numeric_limits<float>::infinity();
      for (int64_t j = beg; j < end; ++j) {
        s[j - beg] = score(r, h, j);
        m = nanmax(m, s[j - beg]);
      }
      float l = 0.0f;
      for (int64_t j = beg; j < end; ++j) {
        const float e = std::exp(s[j - beg] - m);
        const float* vu = val + indices[j] * F + h * D;
        l += e;
        for (int64_t d = 0; d < D; ++d) o[d] += e * vu[d];
      }
      for (int64_t d = 0; d < D; ++d) o[d] = o[d] / l;
      lse[r * H + h] = m + std::log(l);
    }
  }
}

}  // namespace dglhip
