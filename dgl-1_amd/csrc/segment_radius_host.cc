// Segment fixed-radius neighbours on the host: segment_radius.hip's contract
// by the plain loop per query, the queries split over the thread pool. The
// distance is the same float32 chain (t = x_j[c] - q_i[c]; s = fmaf(t, t, s),
// c ascending), membership the same strict d < r2, the walk in row order with
// the same stop at k members and the same padding: the device's bits on every
// input.
#include "../../include/dgl_hip.h"
#include "common.h"

#include <cmath>
#include <limits>

using namespace dglhip;

namespace {

void check_offsets(const char* what, const int64_t* offsets, int64_t B, int64_t rows) {
  DGLHIP_CHECK(offsets != nullptr, what << " offsets is null");
  DGLHIP_CHECK(offsets[0] == 0, what << " offsets must start at 0, got " << offsets[0]);
  for (int64_t s = 0; s < B; ++s)
    DGLHIP_CHECK(offsets[s + 1] >= offsets[s], what << " offsets decrease at segment " << s);
  DGLHIP_CHECK(offsets[B] == rows, what << " offsets end at " << offsets[B] << ", expected the "
                                        << rows << " rows");
}

}  // namespace

extern "C" {

int dglhip_segment_radius_host(int64_t num_segments, int64_t num_rows, int64_t num_queries,
                               int64_t dim, int64_t k, float r2, int flags,
                               const int64_t* x_offsets, const float* x, int64_t ldx,
                               const int64_t* q_offsets, const float* q, int64_t ldq,
                               int64_t* nbr, int32_t* cnt, float* dist, int num_threads) {
  API_BEGIN();
  const int64_t B = num_segments, N = num_rows, M = num_queries, D = dim;
  DGLHIP_CHECK(B >= 0 && N >= 0 && M >= 0, "negative size");
  DGLHIP_CHECK(k >= 1 && k <= DGLHIP_RADIUS_MAX_K,
               "k = " << k << " outside [1, DGLHIP_RADIUS_MAX_K = " << DGLHIP_RADIUS_MAX_K << "]");
  DGLHIP_CHECK(D >= 1 && D <= DGLHIP_RADIUS_MAX_DIM,
               "D = " << D << " outside [1, DGLHIP_RADIUS_MAX_DIM = " << DGLHIP_RADIUS_MAX_DIM
                      << "]");
  DGLHIP_CHECK(N < (int64_t(1) << 31) && M < (int64_t(1) << 31),
               "num_rows and num_queries must be below 2^31");
  DGLHIP_CHECK((flags & ~(DGLHIP_RADIUS_EXCLUDE_SELF | DGLHIP_RADIUS_PAD_FIRST)) == 0,
               "unknown flags " << flags);
  check_offsets("x", x_offsets, B, N);
  check_offsets("q", q_offsets, B, M);
  if (B == 0 || M == 0) return 0;
  DGLHIP_CHECK(q && nbr && cnt && (N == 0 || x), "null pointer argument");
  DGLHIP_CHECK(ldx >= D && ldq >= D, "row stride below the row width");
  const bool skip = (flags & DGLHIP_RADIUS_EXCLUDE_SELF) != 0;
  const bool pad_first = (flags & DGLHIP_RADIUS_PAD_FIRST) != 0;
  const int nt = num_threads > 0 ? num_threads : default_num_threads();
  const float inf = std::numeric_limits<float>::infinity();
  // the segment of every query, so that the queries (not the segments) are split
  std::vector<int64_t> seg(M);
  for (int64_t s = 0; s < B; ++s)
    std::fill(seg.begin() + q_offsets[s], seg.begin() + q_offsets[s + 1], s);
  parallel_for(M, nt, [&](int64_t i0, int64_t i1, int) {
    float dq[DGLHIP_RADIUS_MAX_K];
    for (int64_t i = i0; i < i1; ++i) {
      const int64_t beg = x_offsets[seg[i]], end = x_offsets[seg[i] + 1];
      const float* qi = q + i * ldq;
      int64_t* ni = nbr + i * k;
      int64_t n = 0;
      for (int64_t j = beg; j < end && n < k; ++j) {
        if (skip && j == i) continue;
        const float* xj = x + j * ldx;
        float d = 0.0f;
        for (int64_t c = 0; c < D; ++c) {
          const float t = xj[c] - qi[c];
          d = std::fmaf(t, t, d);
        }
        if (d < r2) {  // strictly; a NaN is outside
          ni[n] = j;
          dq[n++] = d;
        }
      }
      cnt[i] = static_cast<int32_t>(n);
      const bool pad = pad_first && n > 0;
      for (int64_t j = n; j < k; ++j) {
        ni[j] = pad ? ni[0] : -1;
        dq[j] = pad ? dq[0] : inf;
      }
      if (dist != nullptr) std::copy(dq, dq + k, dist + i * k);
    }
  }, 16);
  API_END();
}

}  // extern "C"
