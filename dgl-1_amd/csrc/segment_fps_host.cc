// Segment farthest point sampling on the host: segment_fps.hip's contract by
// the plain loop, the segments split over the thread pool. The distance is
// the same float32 chain (t = x_j[c] - x_p[c]; s = fmaf(t, t, s), c ascending),
// the running minimum the same compare and the pick the same strict order
// (largest minimum, lowest row), so the bits are the device's on every input.
#include "../../include/dgl_hip.h"
#include "common.h"

#include <cmath>
#include <limits>

using namespace dglhip;

extern "C" {

int dglhip_segment_fps_host(int64_t num_segments, int64_t num_rows, int64_t dim, int64_t m,
                            const int64_t* offsets, const float* x, int64_t ldx,
                            const int64_t* start, int64_t* idx, float* dist, int num_threads) {
  API_BEGIN();
  const int64_t B = num_segments, N = num_rows, D = dim;
  DGLHIP_CHECK(B >= 0 && N >= 0, "negative size");
  DGLHIP_CHECK(m >= 1, "m = " << m << " picks");
  DGLHIP_CHECK(D >= 1 && D <= DGLHIP_FPS_MAX_DIM,
               "D = " << D << " outside [1, DGLHIP_FPS_MAX_DIM = " << DGLHIP_FPS_MAX_DIM << "]");
  DGLHIP_CHECK(N < (int64_t(1) << 31), "num_rows must be below 2^31");
  DGLHIP_CHECK(offsets != nullptr, "offsets is null");
  DGLHIP_CHECK(offsets[0] == 0, "offsets must start at 0, got " << offsets[0]);
  for (int64_t s = 0; s < B; ++s)
    DGLHIP_CHECK(offsets[s + 1] >= offsets[s], "offsets decrease at segment " << s);
  DGLHIP_CHECK(offsets[B] == N, "offsets end at " << offsets[B] << ", expected the " << N
                                                  << " rows");
  if (B == 0) return 0;
  DGLHIP_CHECK(idx && dist && (N == 0 || x), "null pointer argument");
  DGLHIP_CHECK(ldx >= D, "row stride below the row width");
  if (start != nullptr)
    for (int64_t s = 0; s < B; ++s) {
      const int64_t len = offsets[s + 1] - offsets[s];
      DGLHIP_CHECK(len == 0 || (start[s] >= 0 && start[s] < len),
                   "start " << start[s] << " is no row of segment " << s << " of " << len);
    }
  const int nt = num_threads > 0 ? num_threads : default_num_threads();
  const float inf = std::numeric_limits<float>::infinity();
  parallel_for(B, nt, [&](int64_t s0, int64_t s1, int) {
    std::vector<float> mind;  // -1: taken
    for (int64_t s = s0; s < s1; ++s) {
      const int64_t beg = offsets[s], len = offsets[s + 1] - beg;
      const int64_t picks = std::min(m, len);
      int64_t* si = idx + s * m;
      float* sd = dist + s * m;
      for (int64_t j = picks; j < m; ++j) {
        si[j] = -1;
        sd[j] = 0.0f;
      }
      if (len == 0) continue;
      mind.assign(len, inf);
      int64_t win = start != nullptr ? start[s] : 0;
      float dwin = inf;
      for (int64_t i = 0;; ++i) {
        si[i] = beg + win;
        sd[i] = dwin;
        if (i + 1 >= picks) break;
        mind[win] = -1.0f;
        const float* xp = x + (beg + win) * ldx;
        win = -1;
        dwin = -1.0f;
        for (int64_t j = 0; j < len; ++j) {
          if (mind[j] < 0.0f) continue;
          const float* xj = x + (beg + j) * ldx;
          float d = 0.0f;
          for (int64_t c = 0; c < D; ++c) {
            const float t = xj[c] - xp[c];
            d = std::fmaf(t, t, d);
          }
          if (d < mind[j]) mind[j] = d;
          if (mind[j] > dwin) {  // strictly: the lowest row among equals
            dwin = mind[j];
            win = j;
          }
        }
      }
    }
  }, 2);
  API_END();
}

}  // extern "C"
